"""Memory-less automata on strings given in pieces (mfa_match_batch_resume), the part that can be wrong without a GPU
(csrc/dfa_resume_core.h: the state a piece is entered with, the sticky error, the walk of a piece and the fold of chunk maps from a given
state), compiled for the host (tests/emul/dfa_resume_emul.cpp) and run against the CPU restatement; and what the C-ABI answers before it
touches a device.  The kernels around it are checked by tests/test_dfa_resume_gpu.py, on the same corpus (tests/testlib.py)."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import oracle_lib
from mfa_amd import capi, image
from testlib import MAX_BYTES, NFA_NAMES, ROUNDS, blob_of, corpus, cuts_for, emul_exe, out_offsets, rounds_of, seen_so_far, table_66, table_127, write_batch


@pytest.fixture(scope="module")
def emul():
    return emul_exe("dfa_resume")


def run_pieces(emul, tmp_path, blob, data, total, states_in, pairs, form):
    """pairs: rounds x n x (b, e) absolute positions in `data`; returns (states, results) arrays of shape rounds x n"""
    n = len(states_in)
    (tmp_path / "a.blob").write_bytes(blob)
    flat = np.array(pairs, dtype="<u8").reshape(-1)
    (tmp_path / "rounds.bin").write_bytes(struct.pack("<QQ", n, len(pairs)) + np.asarray(states_in, dtype="<u4").tobytes() + flat.tobytes()
                                          + struct.pack("<Q", total) + data.tobytes()[:total])
    p = subprocess.run([emul, "pieces", str(tmp_path / "a.blob"), str(tmp_path / "rounds.bin"), form], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()[-400:]
    rows = [[tuple(int(x) for x in w.split(b":")) for w in line.split()] for line in p.stdout.splitlines()]
    assert len(rows) == len(pairs) and all(len(row) == n for row in rows)
    return np.array([[w[0] for w in row] for row in rows], dtype=np.uint32), np.array([[w[1] for w in row] for row in rows], dtype=np.uint8)


@pytest.mark.parametrize("rev", [0, 1], ids=["forward", "reversed"])
@pytest.mark.parametrize("name", NFA_NAMES)
def test_resume_core_against_oracle(emul, name, rev, tmp_path):
    """every nfa_* fixture, both scan directions, both table forms: after every piece the result is the oracle's on what has been given so
    far, after the last piece state and result are those of the whole string in one piece"""
    blob, strings, is_rev = corpus(name, rev)
    assert is_rev >= rev
    rng = np.random.default_rng(len(name) * 977 + rev)
    cuts = cuts_for(strings, rng)
    off = out_offsets(strings)
    assert {(o + c) % 16 for o, cs in zip(off, cuts) for c in cs[1:-1]} == set(range(16))
    assert any(a == b for cs in cuts for a, b in zip(cs[:-1], cs[1:])) and {len(cs) - 1 for cs in cuts} == {1, 2, 3, 4}
    rounds = rounds_of(strings, cuts, is_rev)
    data, poff = oracle_lib.pack(strings)
    total = int(poff[-1])
    ora = oracle_lib.OracleImage(blob)
    want_whole = ora.match(strings)
    start = [capi.DFA_STATE_START] * len(strings)
    for form in ("lds", "big"):
        whole_st, whole_res = run_pieces(emul, tmp_path, blob, data, total, start, [[(o, o + len(s)) for o, s in zip(off, strings)]], form)
        assert np.array_equal(whole_res[0], want_whole), form
        pairs = [[(o + b, o + e) for o, (b, e) in zip(off, row)] for row in rounds]
        st, res = run_pieces(emul, tmp_path, blob, data, total, start, pairs, form)
        for r in range(ROUNDS):
            want = ora.match(seen_so_far(strings, rounds, r, is_rev))
            bad = np.nonzero(res[r] != want)[0]
            assert bad.size == 0, "%s %s round %d: %d mismatches, first string %d (len %d) want %d" % (name, form, r, bad.size, bad[0], len(strings[bad[0]]), want[bad[0]])
        assert np.array_equal(st[-1], whole_st[0]) and np.array_equal(res[-1], want_whole), form
        assert int(st.max()) < capi.Image(blob).info()["dfa_states"]


def test_sticky_error_and_dead_state(emul, tmp_path):
    """a word that names no state set, the error word itself and a piece of limit + 1 bytes leave the error word and result 2, and so does
    a valid piece after that; the dead state stays dead with result 0; the neighbours are walked"""
    blob = blob_of("nfa_abb_thompson", 0)
    states = capi.Image(blob).info()["dfa_states"]
    text = b"ababb" + b"abb" + b"zabb" + b"abb" + b"abb"
    data = np.frombuffer(text + bytes(16), dtype=np.uint8)
    # strings: good, bad word, error word, too long (its bytes are never read), dead, good
    first = [(0, 5), (5, 8), (5, 8), (0, MAX_BYTES + 1), (5, 8), (5, 8)]
    second = [(5, 8), (5, 8), (5, 8), (5, 8), (5, 8), (8, 12)]
    st_in = [capi.DFA_STATE_START, states, capi.DFA_STATE_INVALID, capi.DFA_STATE_START, capi.DFA_STATE_DEAD, capi.DFA_STATE_START]
    for form in ("lds", "big"):
        st, res = run_pieces(emul, tmp_path, blob, data, len(text), st_in, [first, second], form)
        for r in range(2):
            assert list(st[r][1:4]) == [capi.DFA_STATE_INVALID] * 3 and list(res[r][1:4]) == [2, 2, 2]
            assert st[r][4] == capi.DFA_STATE_DEAD and res[r][4] == 0
        assert list(res[:, 0]) == [1, 1] and list(res[:, 5]) == [1, 0] and st[1][5] == capi.DFA_STATE_DEAD
        # exactly the limit is no error (entered dead, so the harness reads nothing)
        st, res = run_pieces(emul, tmp_path, blob, data, len(text), [capi.DFA_STATE_DEAD], [[(0, MAX_BYTES)]], form)
        assert (int(st[0][0]), int(res[0][0])) == (capi.DFA_STATE_DEAD, 0)


@pytest.mark.parametrize("rev", [0, 1], ids=["forward", "reversed"])
@pytest.mark.parametrize("states", [66, 127])
def test_fold_from_every_start_state(emul, states, rev, tmp_path):
    """chunk maps composed as the fold kernel composes them (tiles of maps, runs side by side, one lane through the runs), started from
    EVERY state set of a 66- and a 127-state-set table, against the plain byte-by-byte walk of the table from that state"""
    blob = table_66(tmp_path, rev) if states == 66 else table_127(tmp_path, rev)
    assert image.blob_info(blob)["reversed"] == rev and capi.Image(blob).info()["dfa_states"] == states
    rng = np.random.default_rng(states + rev)
    alpha = np.frombuffer(b"ab" if states == 66 else b"aabbcd", dtype=np.uint8)
    strings = [alpha[rng.integers(0, len(alpha), size=int(ln))].tobytes() for ln in [0, 1, 15, 16, 17, 255, 4096, 5000] + [int(x) for x in rng.integers(0, 3000, size=20)]]
    strings += [alpha[rng.integers(0, 2, size=900)].tobytes() + b"abbbbbcdcdcdcccc", b"ab" * 700 + b"abbbbb"]
    if rev:
        strings = [s[::-1] for s in strings]
    (tmp_path / "a.blob").write_bytes(blob)
    write_batch(tmp_path / "batch.bin", strings)
    for chunk, tile in ((16, 2048), (48, 512), (256, 32768), (4096, 32768)):
        p = subprocess.run([emul, "fold", str(tmp_path / "a.blob"), str(tmp_path / "batch.bin"), str(chunk), str(tile)], capture_output=True)
        assert p.returncode == 0, p.stderr.decode()[-400:]
        assert p.stdout.split() == [b"ok", b"%d" % states, b"%d" % (states * len(strings))]


# ---- the C-ABI, before it touches a device ------------------------------------------------------------------------------------------
def _resume(img, states_ptr, n=1, device=0):
    buf = (ctypes.c_uint8 * 64)()
    off = (ctypes.c_uint64 * 2)(0, 3)
    res = (ctypes.c_uint8 * 4)()
    L = capi.lib()
    return (L.mfa_match_batch_resume(img._h, buf, off, n, states_ptr, res, device, None),
            L.mfa_match_batch_resume_host(img._h, buf, off, n, states_ptr, res, device))


def test_resume_errors_without_a_device():
    st = (ctypes.c_uint32 * 4)(1, 1, 1, 1)
    mem = capi.Image(image.blob_from_dump(oracle_lib.load_dump("ex1_plain")))
    assert _resume(mem, st) == (capi.ERR_UNSUPPORTED, capi.ERR_UNSUPPORTED)
    nfa = capi.Image(image.blob_from_dump(oracle_lib.load_dump("nfa_abb_thompson")))
    assert _resume(nfa, None) == (capi.ERR_INVALID_ARG, capi.ERR_INVALID_ARG)
    assert _resume(nfa, st, n=0) == (capi.OK, capi.OK)
    # no such device: device 0 on a machine without a GPU, one past the last otherwise -- the call never reaches a kernel
    count = capi.device_count()
    assert _resume(nfa, st, device=max(count, 0)) == (capi.ERR_NO_DEVICE, capi.ERR_NO_DEVICE)
    assert list(st) == [1, 1, 1, 1]
    with pytest.raises(capi.MfaError) as e:
        mem.match_host_resume(np.zeros(16, dtype=np.uint8), np.array([0, 3], dtype=np.uint64), np.ones(1, dtype=np.uint32))
    assert e.value.code == capi.ERR_UNSUPPORTED


def test_strerror_is_unchanged():
    want = ["ok", "invalid argument", "malformed automaton image blob", "automaton outside the limits of the device kernels",
            "no usable HIP device (there is no CPU fallback)", "HIP runtime error", "out of host memory",
            "string longer than MFA_MAX_STRING_BYTES", "compiling the specialised kernel failed", "unknown error"]
    assert [capi.lib().mfa_strerror(-k).decode() for k in range(10)] == want


def test_constants_equal_the_header():
    hdr = open(os.path.join(oracle_lib.ROOT, "include", "mfa_hip.h")).read()
    got = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define\s+MFA_DFA_STATE_(\w+)\s+(0x[0-9a-fA-F]+|\d+)u", hdr)}
    assert got == {"DEAD": capi.DFA_STATE_DEAD, "START": capi.DFA_STATE_START, "INVALID": capi.DFA_STATE_INVALID}
    assert (capi.DFA_STATE_DEAD, capi.DFA_STATE_START, capi.DFA_STATE_INVALID) == (0, 1, 0xffffffff)
    assert int(re.search(r"#define\s+MFA_MAX_STRING_BYTES\s+(0x[0-9a-fA-F]+)u", hdr).group(1), 16) == MAX_BYTES == 0x00ffffff
