"""Set-walk images on strings given in pieces, the part that can be wrong without a GPU (csrc/nfa_set_core.h: the record that carries a
string's set of live nodes from call to call, its decode and check, the walk of one piece from a given set, its encode), compiled for
the host (tests/emul/nfa_set_resume_emul.cpp) and run against the CPU restatement, against whole walks and against the tabulated step
function; and what mfa_match_batch_resume_set answers before it touches a device.  The kernel around it is checked by
tests/test_nfa_set_resume_gpu.py, on the same corpus and the same cuts (tests/testlib.py, tests/setwalk_lib.py)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib
from mfa_amd import capi, image
from setwalk_lib import INVALID, LANE_WORDS, LIVE, START, check_records_are_clean, mask_words, piece_rounds, record, run_lane_pieces, run_lane_table, whole
from testlib import MAX_BYTES, NFA_NAMES, ROUNDS, blob_of, emul_exe, expected, out_offsets, seen_so_far, setwalk_corpus, wide_images, wide_strings


@pytest.fixture(scope="module")
def emul():
    return emul_exe("nfa_set_resume")


def pieces_against_whole(emul, tmp_path, blob, strings, want, rng, what):
    """the strings cut by testlib.cuts_for and fed in ROUNDS rounds in scan order: every round's digits are the oracle's answers on what has
    been given so far, the final records are those of the whole strings in one round, and those are clean"""
    rounds, is_rev = piece_rounds(blob, strings, rng)
    cuts = {(k, b) for row in rounds for k, (b, e) in enumerate(row)}
    off = out_offsets(strings)
    assert {(off[k] + b) % 16 for k, b in cuts} == set(range(16))                     # a cut at every residue mod 16 of the buffer
    assert any(b == e and len(s) for row in rounds for s, (b, e) in zip(strings, row))      # empty pieces of strings that are not
    digits, recs = run_lane_pieces(emul, tmp_path, blob, strings, rounds)
    ora = oracle_lib.OracleImage(blob)
    for r in range(ROUNDS):
        ref = want if r == ROUNDS - 1 else ora.match(seen_so_far(strings, rounds, r, is_rev))
        bad = np.nonzero(digits[r] != ref)[0]
        assert bad.size == 0, "%s round %d: %d mismatches, first string %d (len %d) want %d got %d" % (what, r, bad.size, bad[0], len(strings[bad[0]]), ref[bad[0]], digits[r][bad[0]])
    whole_digits, whole_recs = run_lane_pieces(emul, tmp_path, blob, strings, whole(strings))
    assert np.array_equal(whole_digits[0], want), what
    assert np.array_equal(recs, whole_recs), what
    check_records_are_clean(recs, image.blob_info(blob)["n_nodes"], LANE_WORDS)
    assert (recs[:, 0] == LIVE).all()
    return recs


@pytest.mark.parametrize("rev", [0, 1], ids=["forward", "reversed"])
@pytest.mark.parametrize("name", NFA_NAMES)
def test_pieces_on_the_harness(emul, env, name, rev, tmp_path):
    blob, strings, golden = setwalk_corpus(name, rev)
    want = expected(blob, strings, golden)
    recs = pieces_against_whole(emul, tmp_path, blob, strings, want, np.random.default_rng(len(name) * 977 + rev), "%s rev %d" % (name, rev))
    assert recs[want == 1, 4:].any(axis=1).all()                                   # an accepted string's set is not empty
    # whole walks against the table: the final set is, bit for bit, the node set the table's state names
    n, states, W = run_lane_table(emul, tmp_path, blob, strings)
    assert (n, W) == (len(strings), mask_words(image.blob_info(blob)["n_nodes"])) and states == capi.Image(blob).info()["dfa_states"]


def test_wider_masks_and_deep_chains(emul, tmp_path):
    """two, four and eight mask words, and epsilon chains that need the stack"""
    rng = np.random.default_rng(79)
    seen_w = set()
    for key, blob in wide_images(tmp_path).items():
        strings = wide_strings(rng)
        want = oracle_lib.OracleImage(blob).match(strings)
        assert 0 < int(want.sum()) < len(strings), key
        pieces_against_whole(emul, tmp_path, blob, strings, want, rng, key)
        n, _, W = run_lane_table(emul, tmp_path, blob, strings)
        assert n == len(strings) and W == mask_words(image.blob_info(blob)["n_nodes"])
        seen_w.add(W)
    assert {2, 4, 8} <= seen_w


# ---- the record's checks ------------------------------------------------------------------------------------------------------------------
def test_record_checks_on_the_harness(emul, tmp_path):
    """every sticky-error cause that needs no 16 MiB of input -- an unknown tag, INVALID on entry, a reserved word, a bit for a node the
    image lacks inside its mask width and in a word beyond it, a piece of limit + 1 bytes (not walked, so it needs no bytes) -- gives
    INVALID, zero nodes and 2, and stays so after a valid piece; a START record with garbage in `nodes` equals a zeroed one; dead on entry
    leaves dead with result 0"""
    blob = blob_of("nfa_abb_thompson", 0)
    n_nodes = image.blob_info(blob)["n_nodes"]
    assert n_nodes < 32 and not image.blob_info(blob)["reversed"]
    text = b"ababb"
    ok = record(LANE_WORDS, START)
    rows = [record(LANE_WORDS, 2), record(LANE_WORDS, INVALID), record(LANE_WORDS, LIVE, [1], (0, 5, 0)), record(LANE_WORDS, START, [], (1, 0, 0)),
            record(LANE_WORDS, LIVE, [1 << n_nodes]), record(LANE_WORDS, LIVE, [1, 1]), record(LANE_WORDS, LIVE, [1, 0, 0, 0, 0, 0, 0, 1 << 31]), ok,
            record(LANE_WORDS, START, [0xdeadbeef] * 8), ok, record(LANE_WORDS, LIVE), ok]
    n = len(rows)
    strings = [text] * n
    first = [(0, 2)] * n
    first[9] = (0, MAX_BYTES + 1)                                                  # a piece of limit + 1 bytes
    digits, recs = run_lane_pieces(emul, tmp_path, blob, strings, [first, [(2, 5)] * n], np.stack(rows))
    errors = [0, 1, 2, 3, 4, 5, 6, 9]
    want_first = np.array([2] * 7 + [0, 0, 2, 0, 0], dtype=np.uint8)               # "ab" is not accepted
    want_last = np.array([2] * 7 + [1, 1, 2, 0, 1], dtype=np.uint8)                # "ababb" is; the dead record stays dead
    assert list(digits[0]) == list(want_first) and list(digits[1]) == list(want_last)
    assert (recs[errors, 0] == INVALID).all() and not recs[errors, 1:].any()
    check_records_are_clean(recs, n_nodes, LANE_WORDS)
    assert np.array_equal(recs[7], recs[8]) and np.array_equal(recs[7], recs[11]) and recs[7, 0] == LIVE and recs[7, 4] != 0
    assert list(recs[10]) == [LIVE] + [0] * 11
    # the same first round alone: the errors are errors at once, not only after the second piece
    _, recs1 = run_lane_pieces(emul, tmp_path, blob, strings, [first], np.stack(rows))
    assert (recs1[errors, 0] == INVALID).all() and not recs1[errors, 1:].any() and list(recs1[10]) == [LIVE] + [0] * 11


def test_a_record_of_nodes_no_walk_reaches_together_is_safe(emul, tmp_path):
    """EVERY node of the deep image at once, a set no input leads to: the walk's stack either holds it or answers with the sticky error;
    nothing is read or written out of bounds (the harness under sanitizers, test_harness_under_sanitizers, walks the same record)"""
    blob = wide_images(tmp_path)["deep"]
    n_nodes = image.blob_info(blob)["n_nodes"]
    full = [0xffffffff] * (n_nodes // 32) + ([(1 << (n_nodes % 32)) - 1] if n_nodes % 32 else [])
    digits, recs = run_lane_pieces(emul, tmp_path, blob, [b"abcabc"], whole([b"abcabc"]), np.stack([record(LANE_WORDS, LIVE, full)]))
    assert digits[0][0] in (0, 1, 2)
    check_records_are_clean(recs, n_nodes, LANE_WORDS)
    assert (recs[0, 0] == INVALID) == (digits[0][0] == 2)


def test_harness_under_sanitizers(tmp_path):
    """the harness once more with -fsanitize=address,undefined, a stand-alone program: pieces of one fixture in the room the read rule
    gives and not a byte more, the record checks, and a record that names every node"""
    exe = emul_exe("nfa_set_resume", "-fsanitize=address,undefined -fno-sanitize-recover=all")
    blob, strings, golden = setwalk_corpus("nfa_star4_ssnf", 1)
    want = expected(blob, strings, golden)
    pieces_against_whole(exe, tmp_path, blob, strings, want, np.random.default_rng(3), "nfa_star4_ssnf under sanitizers")
    run_lane_table(exe, tmp_path, blob, strings)
    test_record_checks_on_the_harness(exe, tmp_path)
    test_a_record_of_nodes_no_walk_reaches_together_is_safe(exe, tmp_path)


# ---- the C-ABI, before a device is touched -------------------------------------------------------------------------------------------------
@pytest.fixture()
def env(monkeypatch):
    for k in ("MFA_NFA_SETWALK", "MFA_DFA_STATE_LIMIT"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def test_before_the_device(env):
    """a tabulated image and a memory automaton: MFA_ERR_UNSUPPORTED; NULL states and a state pointer that is not 16-byte aligned:
    MFA_ERR_INVALID_ARG; n == 0: MFA_OK; none of them looks for a device.  A valid call on a machine without one: MFA_ERR_NO_DEVICE"""
    L = capi.lib()
    abb = blob_of("nfa_abb_thompson", 0)
    tab = capi.Image(abb)
    mem = capi.Image(image.blob_from_dump(oracle_lib.load_dump("ex1_plain")))
    env.setenv("MFA_NFA_SETWALK", "1")
    sw = capi.Image(abb)
    assert (tab.info()["dfa_states"], sw.info()["dfa_states"]) == (6, 0)
    buf, off, res = (ctypes.c_uint8 * 64)(), (ctypes.c_uint64 * 2)(0, 3), (ctypes.c_uint8 * 4)()
    st = (ctypes.c_uint32 * (LANE_WORDS + 8))()
    at = ctypes.addressof(st)
    at += -at % 16                                                                  # a 16-byte aligned record inside st
    for img in (tab, mem):
        assert L.mfa_match_batch_resume_set(img._h, buf, off, 1, at, res, 0, None) == capi.ERR_UNSUPPORTED
        assert L.mfa_match_batch_resume_set_host(img._h, buf, off, 1, at, res, 0) == capi.ERR_UNSUPPORTED
    assert L.mfa_match_batch_resume_set(sw._h, buf, off, 1, None, res, 0, None) == capi.ERR_INVALID_ARG
    assert L.mfa_match_batch_resume_set_host(sw._h, buf, off, 1, None, res, 0) == capi.ERR_INVALID_ARG
    assert L.mfa_match_batch_resume_set(sw._h, buf, None, 1, at, res, 0, None) == capi.ERR_INVALID_ARG
    assert L.mfa_match_batch_resume_set(None, buf, off, 1, at, res, 0, None) == capi.ERR_INVALID_ARG
    assert L.mfa_match_batch_resume_set(sw._h, buf, off, 1, at + 4, res, 0, None) == capi.ERR_INVALID_ARG      # a device pointer value off by 4
    assert L.mfa_match_batch_resume_set(sw._h, buf, off, 0, at, res, 0, None) == capi.OK
    assert L.mfa_match_batch_resume_set_host(sw._h, buf, off, 0, at, res, 0) == capi.OK
    assert not any(st) and sw.info()["last_kernel"] == capi.KERNEL_NONE


def test_no_device(env):
    if capi.device_count() > 0:
        pytest.skip("a device is present: the valid call is tests/test_nfa_set_resume_gpu.py's")
    env.setenv("MFA_NFA_SETWALK", "1")
    sw = capi.Image(blob_of("nfa_abb_thompson", 0))
    states = np.zeros(LANE_WORDS, dtype=np.uint32)
    data, off = oracle_lib.pack([b"abb"])
    with pytest.raises(capi.MfaError) as e:
        sw.match_host_resume_set(np.concatenate([data, np.zeros(16, np.uint8)]), off, states)
    assert e.value.code == capi.ERR_NO_DEVICE and not states.any()


def test_constants_equal_the_header(tmp_path):
    hdr_path = os.path.join(oracle_lib.ROOT, "include", "mfa_hip.h")
    hdr = open(hdr_path).read()
    got = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define\s+MFA_SET_STATE_(\w+)\s+(0x[0-9a-fA-F]+|\d+)u", hdr)}
    assert got == {"START": capi.SET_STATE_START, "LIVE": capi.SET_STATE_LIVE, "INVALID": capi.SET_STATE_INVALID}
    assert (capi.SET_STATE_START, capi.SET_STATE_LIVE, capi.SET_STATE_INVALID, capi.SET_STATE_WORDS) == (0, 1, 0xffffffff, 12)
    # sizeof(mfa_set_state) and where its members lie, as a C compiler sees the header
    (tmp_path / "size.c").write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mfa_hip.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(mfa_set_state), '
                                     'offsetof(mfa_set_state, reserved), offsetof(mfa_set_state, nodes)); return 0; }\n')
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.dirname(hdr_path), "-o", str(tmp_path / "size"), str(tmp_path / "size.c")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    out = subprocess.run([str(tmp_path / "size")], capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [48, 4, 16] and 48 == 4 * capi.SET_STATE_WORDS
    assert {"mfa_match_batch_resume_set", "mfa_match_batch_resume_set_host"} <= set(capi.EXPORTS)
