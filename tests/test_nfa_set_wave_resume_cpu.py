"""Wave images on strings given in pieces, the part that can be wrong without a GPU (csrc/nfa_set_wave_core.h: the record of 68 words that
carries a string's node set, across the lanes, from call to call; its decode and check, the walk of one piece from the set it holds, its
encode), compiled for the host (tests/emul/nfa_set_wave_resume_emul.cpp with the 64-lane primitives of tests/emul/wave_lanes.h and
wave_lanes_resume.h) and run against the CPU restatement, against whole walks and against the tabulated step function; and what
mfa_match_batch_resume_set_wide and mfa_image_resume_state_bytes answer before they touch a device.  The kernel around it is checked by
tests/test_nfa_set_wave_resume_gpu.py, on the same images, strings and cuts (tests/setwalk_lib.py)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib
from mfa_amd import capi, image
from setwalk_lib import (COUNTER300, GUARD, LIVE, N_ROUNDS, RAW_NODES, WAVE_MAX_NODES, WIDE_WORDS, check_records_are_clean, check_sticky, fixed_cuts, pieces_of,
                         raw_corpus_once, regex_strings, run_wide_pieces, run_wide_table, sticky_case, three_rounds, wide_regex_images, words_of)
from testlib import blob_of, emul_exe, front_end_blob, seen_so_far

REGEX_IMAGES = ("k_512", "k_512_rev", "k_1024", "k_2048", "deep")


@pytest.fixture(scope="module")
def emul():
    return emul_exe("nfa_set_wave_resume")


@pytest.fixture()
def env(monkeypatch):
    for k in ("MFA_NFA_SETWALK", "MFA_DFA_STATE_LIMIT", "MFA_SET_WAVE"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


# ---- the C-ABI, before a device is touched -------------------------------------------------------------------------------------------------
def test_before_the_device(env, tmp_path):
    """mfa_image_resume_state_bytes names the resume call of every kind of image; the wide call takes the two wave images (n == 0: MFA_OK
    before a device is looked for) and refuses the others with records, guard words and result bytes as they came; NULL or unaligned
    records are MFA_ERR_INVALID_ARG"""
    L = capi.lib()
    abb = blob_of("nfa_abb_thompson", 0)
    mem = capi.Image(image.blob_from_dump(oracle_lib.load_dump("ex1_plain")))
    tab = capi.Image(abb)
    env.setenv("MFA_NFA_SETWALK", "1")
    lane = capi.Image(abb)
    env.setenv("MFA_SET_WAVE", "1")
    wave = capi.Image(abb)
    env.delenv("MFA_SET_WAVE")
    env.delenv("MFA_NFA_SETWALK")
    env.setenv("MFA_DFA_STATE_LIMIT", "100")
    counter = capi.Image(front_end_blob(COUNTER300, tmp_path))
    env.delenv("MFA_DFA_STATE_LIMIT")
    assert counter.info()["n_nodes"] == 303 and counter.info()["dfa_states"] == 0
    assert [im.resume_state_bytes() for im in (mem, tab, lane, wave, counter)] == [0, 4, 48, 272, 272]
    assert 272 == 4 * WIDE_WORDS == 4 * capi.SET_STATE_WIDE_WORDS
    out = ctypes.c_uint32(77)
    assert L.mfa_image_resume_state_bytes(None, ctypes.byref(out)) == capi.ERR_INVALID_ARG
    assert L.mfa_image_resume_state_bytes(wave._h, None) == capi.ERR_INVALID_ARG and out.value == 77
    buf, off = (ctypes.c_uint8 * 64)(), (ctypes.c_uint64 * 2)(0, 3)
    res = (ctypes.c_uint8 * 4)(7, 7, 7, 7)
    st = (ctypes.c_uint32 * (WIDE_WORDS + 8))(*([GUARD] * (WIDE_WORDS + 8)))
    at = ctypes.addressof(st)
    at += -at % 16                                                                  # a 16-byte aligned record inside st, guard words around it
    for img in (wave, counter):
        assert L.mfa_match_batch_resume_set_wide(img._h, buf, off, 0, at, res, 0, None) == capi.OK
        assert L.mfa_match_batch_resume_set_wide_host(img._h, buf, off, 0, at, res, 0) == capi.OK
        assert L.mfa_match_batch_resume_set_wide(img._h, buf, off, 1, None, res, 0, None) == capi.ERR_INVALID_ARG
        assert L.mfa_match_batch_resume_set_wide_host(img._h, buf, off, 1, None, res, 0) == capi.ERR_INVALID_ARG
        assert L.mfa_match_batch_resume_set_wide(img._h, buf, None, 1, at, res, 0, None) == capi.ERR_INVALID_ARG
        assert L.mfa_match_batch_resume_set_wide(img._h, buf, off, 1, at + 4, res, 0, None) == capi.ERR_INVALID_ARG      # a device pointer value off by 4
        assert L.mfa_match_batch_resume_set_wide(img._h, buf, off, 0, at + 8, res, 0, None) == capi.ERR_INVALID_ARG
    assert L.mfa_match_batch_resume_set_wide(None, buf, off, 1, at, res, 0, None) == capi.ERR_INVALID_ARG
    for img in (mem, tab, lane):
        assert L.mfa_match_batch_resume_set_wide(img._h, buf, off, 1, at, res, 0, None) == capi.ERR_UNSUPPORTED
        assert L.mfa_match_batch_resume_set_wide_host(img._h, buf, off, 1, at, res, 0) == capi.ERR_UNSUPPORTED
        assert L.mfa_match_batch_resume_set_wide(img._h, buf, off, 0, at, res, 0, None) == capi.ERR_UNSUPPORTED          # (refused before n is looked at)
        assert L.mfa_match_batch_resume_set_wide(img._h, buf, off, 1, None, res, 0, None) == capi.ERR_INVALID_ARG
    assert list(st) == [GUARD] * (WIDE_WORDS + 8) and list(res) == [7, 7, 7, 7]
    assert all(im.info()["last_kernel"] == capi.KERNEL_NONE for im in (mem, tab, lane, wave, counter))


def test_constants_equal_the_header(tmp_path):
    hdr_path = os.path.join(oracle_lib.ROOT, "include", "mfa_hip.h")
    (tmp_path / "size.c").write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mfa_hip.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(mfa_set_state_wide), '
                                     'offsetof(mfa_set_state_wide, reserved), offsetof(mfa_set_state_wide, nodes)); return 0; }\n')
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.dirname(hdr_path), "-o", str(tmp_path / "size"), str(tmp_path / "size.c")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    out = subprocess.run([str(tmp_path / "size")], capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [272, 4, 16] and capi.SET_STATE_WIDE_WORDS == 68
    assert {"mfa_match_batch_resume_set_wide", "mfa_match_batch_resume_set_wide_host", "mfa_image_resume_state_bytes"} <= set(capi.EXPORTS)
    core = open(os.path.join(oracle_lib.ROOT, "re2-modification_amd", "csrc", "nfa_set_wave_core.h")).read()
    assert re.search(r"kWaveStateWords = 4u \+ kWaveLanes;", core) and re.search(r"kWaveLanes = 64;", core)


# ---- pieces equal whole ---------------------------------------------------------------------------------------------------------------------
def pieces_against_whole(emul, tmp_path, blob, strings, rounds, is_rev, want, what):
    """the strings fed in N_ROUNDS rounds in scan order: EVERY round's digits are the oracle's answers on what has been given so far, the
    final records are bit for bit those of the whole strings in one round, and those are clean.  Returns (tables, records)"""
    assert len(rounds) == N_ROUNDS
    tables, digits, recs = run_wide_pieces(emul, tmp_path, blob, [pieces_of(strings, row) for row in rounds])
    ora = oracle_lib.OracleImage(blob)
    for r in range(N_ROUNDS):
        ref = want if r == N_ROUNDS - 1 else ora.match(seen_so_far(strings, rounds, r, is_rev))
        bad = np.nonzero(digits[r] != ref)[0]
        assert bad.size == 0, "%s round %d: %d mismatches, first string %d (len %d) want %d got %d" % (what, r, bad.size, bad[0], len(strings[bad[0]]), ref[bad[0]], digits[r][bad[0]])
    _, whole_digits, whole_recs = run_wide_pieces(emul, tmp_path, blob, [strings])
    assert np.array_equal(whole_digits[0], want), what
    assert np.array_equal(recs, whole_recs), what
    n_nodes = image.blob_info(blob)["n_nodes"]
    check_records_are_clean(recs, n_nodes, WIDE_WORDS)
    assert (recs[:, 0] == LIVE).all() and tables[1] == words_of(n_nodes)
    assert recs[want == 1, 4:].any(axis=1).all()                                   # an accepted string's set is not empty
    return tables, recs


@pytest.mark.parametrize("name", REGEX_IMAGES)
def test_pieces_on_wide_regex_images(emul, name, tmp_path):
    blob, alphabet, min_len = wide_regex_images(tmp_path)[name]
    rng = np.random.default_rng(len(name))
    strings = regex_strings(rng, alphabet, min_len)
    want = oracle_lib.OracleImage(blob).match(strings)
    assert 0 < int(want.sum()) < len(strings), name
    rounds, is_rev = three_rounds(blob, strings, rng)
    assert is_rev == (1 if name in ("k_512_rev", "deep") else 0)
    assert any(b == e and len(s) for s, (b, e) in zip(strings, rounds[1]))             # empty pieces of strings that are not, in the middle round
    pieces_against_whole(emul, tmp_path, blob, strings, rounds, is_rev, want, name)
    # the fixed cuts: pieces of 0, 1, 15, 16, 17, 1023, 1024 and 1025 bytes, a piece's first byte at every offset mod 16 of a round's buffer
    pick = lambda ln: bytes(rng.choice(list(alphabet), size=int(ln)).tolist())
    strings, rounds = fixed_cuts(pick, is_rev)
    want = oracle_lib.OracleImage(blob).match(strings)
    assert 0 < int(want.sum()) < len(strings), name
    pieces_against_whole(emul, tmp_path, blob, strings, rounds, is_rev, want, name + ", fixed cuts")


def test_pieces_on_raw_images(emul, tmp_path):
    """raw random images of 257 to 2048 nodes, `finish` anywhere, both scan directions, on strings drawn from the automaton"""
    corpus, dropped = raw_corpus_once()
    assert 10 * dropped <= len(corpus) + dropped and {image.blob_info(b)["n_nodes"] for _, b, _, _ in corpus} == set(RAW_NODES)
    assert {image.blob_info(b)["reversed"] for _, b, _, _ in corpus} == {0, 1}
    for k, (name, blob, strings, want) in enumerate(corpus):
        rounds, is_rev = three_rounds(blob, strings, np.random.default_rng(k))
        pieces_against_whole(emul, tmp_path, blob, strings, rounds, is_rev, want, name)


# ---- sets equal the table -------------------------------------------------------------------------------------------------------------------
def test_sets_equal_the_table(emul, tmp_path):
    """(a^300)*, 303 nodes, W = 10, about 300 state sets: behind every string the record's `nodes` are exactly the node set of the
    tabulated state the string reaches -- the set's content, not only whether it meets the accept mask"""
    blob = front_end_blob(COUNTER300, tmp_path)
    assert image.blob_info(blob)["n_nodes"] == 303
    rng = np.random.default_rng(5)
    strings = [b"a" * int(x) for x in list(range(0, 40)) + [299, 300, 301, 599, 600, 601, 1023, 1024, 1025, 2049] + [int(v) for v in rng.integers(0, 1200, size=60)]]
    strings += [b"a" * 150 + b"b" + b"a" * 149, b"b", b"a" * 300 + b"b"]           # the dead state
    tables, n, states = run_wide_table(emul, tmp_path, blob, strings)
    assert tables[1] == 10 and n == len(strings) and states >= 300 and states == capi.Image(blob).info()["dfa_states"]


# ---- the record's checks ------------------------------------------------------------------------------------------------------------------
def test_record_checks_on_the_harness(emul, tmp_path):
    """every sticky-error cause -- an unknown tag, INVALID on entry, a reserved word, bit 303 of the 303-node image (word 9, bit 15), a bit
    in word 10 and in word 63, a piece of MFA_MAX_STRING_BYTES + 1 bytes given by offsets only -- gives result 2, tag INVALID and zero
    nodes, at once and again after an ordinary piece; a START record with garbage in `nodes` equals a zeroed one; LIVE with the empty
    set leaves LIVE and empty with result 0; the good strings beside them are matched"""
    blob = front_end_blob(COUNTER300, tmp_path)
    assert image.blob_info(blob)["n_nodes"] == 303 and not image.blob_info(blob)["reversed"]
    rows, rounds, _, _, _, _ = sticky_case()
    _, d1, recs1 = run_wide_pieces(emul, tmp_path, blob, rounds[:1], rows)
    _, d2, recs2 = run_wide_pieces(emul, tmp_path, blob, rounds, rows)
    assert np.array_equal(d1[0], d2[0])
    check_sticky(blob, d2, [recs1, recs2], "harness")


# ---- sanitizers ---------------------------------------------------------------------------------------------------------------------------
def test_under_sanitizers(tmp_path):
    """the harness as a stand-alone program under ASan and UBSan (nothing is loaded into Python): k_512 and deep on the fixed cuts, the
    2048-node raw image (lane 63 and the last bit), and the record checks, whose dead and over-long records have offsets outside the
    buffer -- the batch has exactly the room the 16-byte read rule makes readable, the records exactly n * 272 bytes, the stack exactly
    its slots"""
    exe = emul_exe("nfa_set_wave_resume", "-fsanitize=address,undefined -fno-sanitize-recover=all")
    images = wide_regex_images(tmp_path)
    for name in ("k_512", "deep"):
        blob, alphabet, min_len = images[name]
        rng = np.random.default_rng(9)
        pick = lambda ln: bytes(rng.choice(list(alphabet), size=int(ln)).tolist())
        strings, rounds = fixed_cuts(pick, image.blob_info(blob)["reversed"])
        want = oracle_lib.OracleImage(blob).match(strings)
        pieces_against_whole(exe, tmp_path, blob, strings, rounds, image.blob_info(blob)["reversed"], want, name + " under sanitizers")
    name, blob, strings, want = raw_corpus_once()[0][-1]
    assert image.blob_info(blob)["n_nodes"] == WAVE_MAX_NODES
    rounds, is_rev = three_rounds(blob, strings[:80], np.random.default_rng(2))
    pieces_against_whole(exe, tmp_path, blob, strings[:80], rounds, is_rev, want[:80], name + " under sanitizers")
    test_record_checks_on_the_harness(exe, tmp_path)
    assert run_wide_table(exe, tmp_path, front_end_blob(COUNTER300, tmp_path), [b"a" * 300, b"a" * 17, b"", b"ab"])[0][1] == 10
