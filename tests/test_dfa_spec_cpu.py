"""Long strings of memory-less automata whose table lives in L2 (255 state sets and more), the part that can be wrong without a GPU
(csrc/dfa_spec_core.h: the lookback range, the guess from two seeds, when a chunk is walked again, the resolve loop over the chunks'
records, the home state), compiled for the host (tests/emul/dfa_spec_emul.cpp) and run one lane at a time -- round 0, the repair rounds,
resolve -- against a plain walk of the table (inside the harness) and against the CPU restatement.  The kernels around it are checked by
tests/test_dfa_spec_gpu.py, on the same tables (tests/testlib.py: TABLES)."""
import subprocess

import numpy as np
import pytest

import oracle_lib
from mfa_amd import capi
from testlib import TABLES, emul_exe, table_blob, write_batch

CHUNKS = (16, 48, 4096)
LOOKBACKS = (0, 16, 256)
ROUNDS = (0, 1, 3)


def text_for(name, ln, rng, k=0):
    """a string of ln bytes in the table's alphabet, as the forward scan reads it"""
    if name == "counter":
        s = b"a" * ln
        return s[:ln // 2] + b"b" + s[ln // 2 + 1:] if k % 7 == 3 and ln else s        # some die half way
    body = np.frombuffer(b"ab", dtype=np.uint8)[rng.integers(0, 2, size=ln)].tobytes()
    if name == "prefix" and k % 5 != 4:                                               # (every fifth lacks the prefix and dies at once)
        body = (b"xyz" + body)[:ln]
    return body


def lengths_for(name, chunk):
    lens = [0, 1, 15, 16, 17, chunk - 1, chunk, chunk + 1, 5 * chunk + 3]
    if name == "counter":
        lens += [300, 600, 300 * (5 * chunk // 300 + 1)]                                # accepted ones
    return lens


def batch_for(name, chunk, rev, rng):
    """every length at every begin alignment 0..15 (a filler string in front moves the begin where it has to be)"""
    strings, at, want_at = [], 0, []
    for ln in lengths_for(name, chunk):
        for align in range(16):
            fill = (align - at) % 16
            if fill:
                strings.append(text_for(name, fill, rng))
                at += fill
            want_at.append((len(strings), align))
            strings.append(text_for(name, ln, rng, k=len(strings)))
            at += ln
    if rev:
        strings = [s[::-1] for s in strings]
    off = np.concatenate([[0], np.cumsum([len(s) for s in strings])])
    assert all(int(off[i]) % 16 == a for i, a in want_at)
    return strings


@pytest.fixture(scope="module")
def emul():
    return emul_exe("dfa_spec")


def run_emul(emul, tmp_path, chunk, lookback, rounds, mode):
    p = subprocess.run([emul, str(tmp_path / "a.blob"), str(tmp_path / "batch.bin"), str(chunk), str(lookback), str(rounds), mode], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()[-400:]
    head, results = p.stdout.split(b"\n")[:2]
    w = head.split()
    assert w[0] == b"ok"
    keys = ("states", "checks", "rewalked", "serial_strings", "serial_bytes", "home")
    return dict(zip(keys, (int(x) for x in w[1:]))), np.frombuffer(results, dtype=np.uint8) - ord("0")


def write_case(tmp_path, blob, strings):
    (tmp_path / "a.blob").write_bytes(blob)
    write_batch(tmp_path / "batch.bin", strings)


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("rev", [0, 1], ids=["forward", "reversed"])
@pytest.mark.parametrize("name", list(TABLES))
def test_spec_core_against_plain_walk_and_oracle(emul, name, rev, chunk, tmp_path):
    """three tables, both directions, chunks of 16, 48 and 4096 bytes, every length at every begin alignment, lookback 0 / 16 / 256, 0 / 1 / 3
    repair rounds: the state is the plain walk's (checked inside the harness), the result the oracle's"""
    blob = table_blob(name, tmp_path, rev)
    states = capi.Image(blob).info()["dfa_states"]
    assert states >= 255 and states == (TABLES[name][1] or states)
    strings = batch_for(name, chunk, rev, np.random.default_rng(chunk * 7 + rev))
    write_case(tmp_path, blob, strings)
    want = oracle_lib.OracleImage(blob).match(strings)
    assert 0 < want.sum() < len(strings)
    for lookback in LOOKBACKS:
        for rounds in ROUNDS:
            got, res = run_emul(emul, tmp_path, chunk, lookback, rounds, "one")
            assert got["states"] == states and got["checks"] == len(strings) and 0 < got["home"] < states
            bad = np.nonzero(res != want)[0]
            assert bad.size == 0, "%s chunk %d lookback %d rounds %d: %d mismatches, first len %d want %d" % (
                name, chunk, lookback, rounds, bad.size, len(strings[bad[0]]), want[bad[0]])
            if rounds == 0:
                assert got["rewalked"] == 0
            if name == "t514" and lookback >= 16:
                # nine bytes of lookback, or all of the string in front of the chunk, fix the state: every guess is right
                assert (got["rewalked"], got["serial_strings"], got["serial_bytes"]) == (0, 0, 0)
            if name == "counter" and rounds == 0:
                # a position modulo 300 cannot be guessed: with no repair round the resolve step has to walk, and is still exact
                assert got["serial_strings"] > 0 and got["serial_bytes"] > 0
            if name == "prefix":
                assert got["home"] != 1
                if chunk == 4096 and lookback == 256:
                    # a walk from {start} dies on the text in front of every chunk but the first; the home state's does not, and nine bytes fix
                    # it: nothing is left to the serial walk, not even without a repair round.  (Chunks walked again: those behind a chunk
                    # that died -- the strings without the prefix -- which cost no walk.)
                    assert got["serial_strings"] == 0


def test_rounds_shorten_the_serial_walk(emul, tmp_path):
    """the counter table, six chunks per string: without a repair round the resolve step walks everything behind the first chunk, with
    three rounds everything behind the fourth; the answer is the same"""
    blob = table_blob("counter", tmp_path)
    strings = [b"a" * (5 * 4096 + 3)] * 4
    write_case(tmp_path, blob, strings)
    got, res = run_emul(emul, tmp_path, 4096, 256, 0, "one")
    assert got["serial_strings"] == 4 and list(res) == [0] * 4
    got3, res3 = run_emul(emul, tmp_path, 4096, 256, 3, "one")
    # three rounds make chunks 1..3 right; chunks 4 and 5 are left to the resolve step: less to walk, the same answer
    assert got3["serial_strings"] == 4 and 0 < got3["serial_bytes"] < got["serial_bytes"] and got3["rewalked"] > 0 and list(res3) == [0] * 4


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("rev", [0, 1], ids=["forward", "reversed"])
def test_resume_form_from_every_state(emul, rev, chunk, tmp_path):
    """the 514-state table entered from EVERY state set but the dead one, as mfa_match_batch_resume enters a piece"""
    blob = table_blob("t514", tmp_path, rev)
    strings = batch_for("t514", chunk, rev, np.random.default_rng(chunk + rev))
    write_case(tmp_path, blob, strings)
    for lookback, rounds in ((16, 1), (0, 3), (256, 0))[:1 if chunk == 4096 else 3]:      # (4096: 513 walks of half a megabyte each, once)
        got, _ = run_emul(emul, tmp_path, chunk, lookback, rounds, "every")
        assert got["checks"] == 513 * len(strings)
