"""Long strings of set-walk images cut across the GPU, the part that can be wrong without one (csrc/nfa_set_split_core.h: the chunk
records, the guess from two seeds, the lanes of round 0 and of a repair round, the resolve loop over records; csrc/image_host.cpp: the home
set), compiled for the host (tests/emul/nfa_set_split_emul.cpp) and run one lane at a time in the kernels' order.  Inside the harness the
final record of every string is compared, word for word, with nfa_set_walk_from over the whole string from the same set; here the result
bytes are compared with the CPU restatement.  The kernels around it are checked by tests/test_nfa_set_split_gpu.py."""
import numpy as np
import pytest

import oracle_lib
from mfa_amd import image
from setwalk_lib import CHUNKS, COUNTER, LOOKBACKS, PREFIX, REPAIR_ROUNDS, ab_strings, fixture_corpus, k_blob, mask_words, run_lane_split
from testlib import NFA_NAMES, emul_exe, front_end_blob, out_offsets, wide_images, wide_strings


@pytest.fixture(scope="module")
def emul():
    return emul_exe("nfa_set_split")


def check_all(runs, want, strings, what):
    for (chunk, lookback, rounds), got, res in runs:
        bad = np.nonzero(res != want)[0]
        assert bad.size == 0, "%s chunk %d lookback %d rounds %d: %d mismatches, first len %d want %d" % (
            what, chunk, lookback, rounds, bad.size, len(strings[bad[0]]), want[bad[0]])
        assert got["checks"] == len(strings) and got["home_nodes"] > 0
        if rounds == 0:
            assert got["rewalked"] == 0


@pytest.mark.parametrize("rev", [0, 1], ids=["forward", "reversed"])
@pytest.mark.parametrize("name", NFA_NAMES)
def test_fixtures_forced_onto_the_set_walk(emul, name, rev, tmp_path):
    """every memory-less fixture, both directions, chunks of 16 / 32 / 64 bytes, lookback 0 / 8 / 256, 0 / 1 / 3 / 8 repair rounds, lengths
    around multiples of the chunk sizes +-1, strings at every offset mod 16"""
    blob, strings = fixture_corpus(name, rev)
    assert {o % 16 for o in out_offsets(strings)} == set(range(16))
    want = oracle_lib.OracleImage(blob).match(strings)
    if not name.startswith("nfa_dot"):
        assert 0 < int(want.sum()) < len(strings)
    runs = run_lane_split(emul, tmp_path, blob, strings, CHUNKS, LOOKBACKS, REPAIR_ROUNDS)
    assert len(runs) == 36 and runs[0][1]["W"] == mask_words(image.blob_info(blob)["n_nodes"])
    check_all(runs, want, strings, "%s rev %d" % (name, rev))


def test_wider_masks_and_deep_chains(emul, tmp_path):
    """two, four and eight mask words, and epsilon chains that need the stack"""
    rng = np.random.default_rng(83)
    seen_w = set()
    for key, blob in wide_images(tmp_path).items():
        strings = wide_strings(rng, n=120)
        want = oracle_lib.OracleImage(blob).match(strings)
        assert 0 < int(want.sum()) < len(strings), key
        runs = run_lane_split(emul, tmp_path, blob, strings, CHUNKS, LOOKBACKS, REPAIR_ROUNDS)
        check_all(runs, want, strings, key)
        seen_w.add(runs[0][1]["W"])
    assert {2, 4, 8} <= seen_w


@pytest.mark.parametrize("rev", [0, 1], ids=["forward", "reversed"])
@pytest.mark.parametrize("name", ["nfa_abb_thompson", "nfa_star4_ssnf", "nfa_alt3_glushkov"])
def test_resume_form_from_every_node_set(emul, name, rev, tmp_path):
    """entered from every node set tabulate_nfa hands out for the image, and from the empty set, as mfa_match_batch_resume_set enters a piece"""
    blob, strings = fixture_corpus(name, rev)
    want = oracle_lib.OracleImage(blob).match(strings)
    runs = run_lane_split(emul, tmp_path, blob, strings, (16, 64), (0, 256), (0, 3), mode="every")
    for _, got, res in runs:
        assert got["checks"] % len(strings) == 0 and got["checks"] // len(strings) >= 4      # START, the empty set, {start}, and more
        assert np.array_equal(res, want)


# ---- pathologies: slow, never wrong ---------------------------------------------------------------------------------------------------------
def test_counter_is_resolved_serially(emul, tmp_path):
    """(a^250)*: the set is a position modulo 250 and never converges.  Every long string (chunks beyond the reach of the lookback and of
    the repair rounds) is resolved serially, without a repair round and with three; more rounds leave less to walk; the answers are right"""
    blob = front_end_blob(COUNTER, tmp_path)
    assert image.blob_info(blob)["n_nodes"] <= 256
    strings = [b"a" * ln for ln in (1000, 1250, 1500, 2047, 2500)] + [b"a" * 600 + b"b" + b"a" * 600]
    want = oracle_lib.OracleImage(blob).match(strings)
    assert list(want) == [1, 1, 1, 0, 1, 0]
    (_, got0, res0), (_, got3, res3) = run_lane_split(emul, tmp_path, blob, strings, (64,), (8,), (0, 3))
    assert np.array_equal(res0, want) and np.array_equal(res3, want)
    assert got0["W"] == 8 and got0["serial_strings"] == len(strings) and got3["serial_strings"] == len(strings)
    assert got3["rewalked"] > 0 and 0 < got3["serial_bytes"] < got0["serial_bytes"]


def test_literal_prefix_guesses_the_home_set(emul, tmp_path):
    """xyz(a|b)*abb: on the text in front of a chunk a walk from {start} dies (no x), and with 8 bytes of lookback the home set's walk
    lives -- but on text that kills the home set's walk too (a run of z, longer than a chunk and its lookback), the guess is the home set"""
    blob = front_end_blob(PREFIX, tmp_path)
    rng = np.random.default_rng(5)
    body = ab_strings([500, 640, 1000], rng, tail=b"abb")
    strings = [b"xyz" + s for s in body] + [b"xyz" + body[0][:100] + b"z" * 80 + body[0][100:], body[1]]
    want = oracle_lib.OracleImage(blob).match(strings)
    assert list(want) == [1, 1, 1, 0, 0]
    runs = run_lane_split(emul, tmp_path, blob, strings, (64,), (8, 256), (0, 3))
    check_all(runs, want, strings, "prefix")
    # string 3 holds 80 z: a chunk begins behind 8 of them, and both seeds die on those
    assert all(got["home_guesses"] > 0 for _, got, _ in runs)
    # the home set lies inside the loop: 8 bytes in front of a chunk fix the set, and nothing of the accepted strings is left to the serial walk
    three, _ = run_lane_split(emul, tmp_path, blob, strings[:3], (64,), (8,), (0,))[0][1:]
    assert (three["serial_strings"], three["rewalked"], three["home_guesses"]) == (0, 0, 0)


@pytest.mark.parametrize("k", [5, 8, 10])
def test_k_images_need_no_repair(emul, k, tmp_path):
    """(a|b)*a(a|b)^k with lookback 256 and 64-byte chunks: the last k + 1 bytes fix the set, so every guess is right -- 0 chunks walked again,
    0 strings resolved serially (what tests/test_dfa_spec_gpu.py observed for their tabulations)"""
    rng = np.random.default_rng(k)
    strings = ab_strings([1024, 1025, 2048, 3000, 5 * 1024, 63, 64, 65], rng)
    for rev in (0, 1):
        blob = k_blob(k, tmp_path, rev)
        want = oracle_lib.OracleImage(blob).match(strings)
        assert 0 < int(want.sum()) < len(strings)
        for rounds in (0, 3):
            (_, got, res), = run_lane_split(emul, tmp_path, blob, strings, (64,), (256,), (rounds,))
            assert np.array_equal(res, want)
            assert (got["rewalked"], got["serial_strings"], got["serial_bytes"]) == (0, 0, 0)


def test_harness_under_sanitizers(tmp_path):
    """the harness once more with -fsanitize=address,undefined, a stand-alone program: one fixture in each direction in the room the read
    rule gives and not a byte more, the resume form, a wide image and the counter"""
    exe = emul_exe("nfa_set_split", "-fsanitize=address,undefined -fno-sanitize-recover=all")
    for rev in (0, 1):
        blob, strings = fixture_corpus("nfa_star4_ssnf", rev)
        want = oracle_lib.OracleImage(blob).match(strings)
        check_all(run_lane_split(exe, tmp_path, blob, strings, CHUNKS, (0, 8), (0, 3)), want, strings, "nfa_star4_ssnf under sanitizers")
    run_lane_split(exe, tmp_path, blob, strings, (16,), (8,), (1,), mode="every")
    blob = wide_images(tmp_path)["deep"]
    strings = wide_strings(np.random.default_rng(1), n=40)
    check_all(run_lane_split(exe, tmp_path, blob, strings, (16, 64), (8,), (0, 3)), oracle_lib.OracleImage(blob).match(strings), strings, "deep under sanitizers")
    blob = front_end_blob(COUNTER, tmp_path)
    strings = [b"a" * 1000, b"a" * 999]
    check_all(run_lane_split(exe, tmp_path, blob, strings, (64,), (8,), (3,)), np.array([1, 0], dtype=np.uint8), strings, "counter under sanitizers")
