"""The memory-less engines' host-compilable cores on automata nobody has seen before (tests/nfa_fuzz.py: raw random automata with up to 200
byte classes, labels of 0x80 and above, letter edges to lower ranks, and random regexes through every compile of the host front-end), all
against the CPU restatement: the reference's step restated in Python, the set walk's mask step against the table from every state set and
class, the split path, the resume call's pieces and folds, the L2 table's guesses, the multi-table item walk and the set walk's records.
What a corpus must hold -- every packed NLIT, every table size that chooses a kernel, every mask width, both scan directions -- is
asserted from info() and the oracle alone, not hoped for.  MFA_FUZZ_SEEDS=n: n more seeds (MFA_FUZZ_FIRST=k: seeds k .. k + n).  The
kernels around the cores are checked by tests/test_nfa_fuzz_gpu.py on the corpus of seed 0."""
import os
import struct
import subprocess

import numpy as np
import pytest

import nfa_fuzz
import oracle_lib
import setresume_lib
from mfa_amd import capi
from test_dfa_resume_cpu import run_pieces
from test_dfa_spec_cpu import run_emul as run_spec
from testlib import ROUNDS, cuts_for, emul_exe, out_offsets, rounds_of, seen_so_far, write_batch

_first = int(os.environ.get("MFA_FUZZ_FIRST", "0"))
SEEDS = list(range(_first, _first + 1 + int(os.environ.get("MFA_FUZZ_SEEDS", "0"))))

_runs = {"run": 0, "refused": 0}


def harness(cmd):
    """the harness's run; None when it refuses the image (exit 3), which is counted and capped (test_refusals_stay_under_the_cap)"""
    p = subprocess.run([str(c) for c in cmd], capture_output=True)
    _runs["run"] += 1
    if p.returncode == 3:
        _runs["refused"] += 1
        return None
    assert p.returncode == 0, (cmd[0], p.stderr.decode()[-400:])
    return p


def differ(got, im, what):
    bad = np.nonzero(np.asarray(got) != im["want"])[0]
    assert bad.size == 0, "%s, %s: %d of %d strings wrong, first %r (len %d) want %d got %d" % (
        im["what"], what, bad.size, len(im["strings"]), im["strings"][bad[0]][:60], len(im["strings"][bad[0]]), im["want"][bad[0]], got[bad[0]])


def states(im):
    return im["info"]["dfa_states"]


@pytest.mark.parametrize("seed", SEEDS)
def test_the_corpus_is_what_the_tests_count_on(seed):
    c = nfa_fuzz.cpu_corpus(seed)
    nfa_fuzz.report(c, seed)
    nfa_fuzz.check_lines(c)


@pytest.mark.parametrize("seed", SEEDS)
def test_python_step_against_oracle(seed):
    """the third restatement of the reference's step: zero differences on every string"""
    for im in nfa_fuzz.cpu_corpus(seed):
        differ([im["walker"].accepts(s, im["info"]["is_reversed"]) for s in im["strings"]], im, "the step in Python")
        # without its memory, on a few strings: the cache is no part of the restatement
        for s, w in list(zip(im["strings"], im["want"]))[:12]:
            assert nfa_fuzz.accepts(im["E"], im["start"], im["finish"], s[:200], im["info"]["is_reversed"]) == oracle_lib.OracleImage(im["blob"]).match([s[:200]])[0]


@pytest.mark.parametrize("seed", SEEDS)
def test_set_walk_core(seed, tmp_path):
    """nfa_set_emul step -- the mask step against the table from EVERY state set and class -- and match, on every image"""
    emul = emul_exe("nfa_set")
    widths = set()
    for im in nfa_fuzz.cpu_corpus(seed):
        (tmp_path / "a.blob").write_bytes(im["blob"])
        write_batch(tmp_path / "batch.bin", im["strings"])
        if states(im):
            p = harness([emul, "step", tmp_path / "a.blob"])
            if p is not None:
                f = p.stdout.split()
                assert f[0] == b"ok" and (int(f[1]), int(f[2]), int(f[3])) == (states(im), im["info"]["byte_classes"], nfa_fuzz.mask_words(im["info"])), im["what"]
        p = harness([emul, "match", tmp_path / "a.blob", tmp_path / "batch.bin"])
        if p is not None:
            differ(np.frombuffer(p.stdout.strip(), dtype=np.uint8) - ord("0"), im, "nfa_set_emul match")
            widths.add((nfa_fuzz.mask_words(im["info"]), im["info"]["is_reversed"]))
    assert widths == {(w, r) for w in (1, 2, 4, 8) for r in (0, 1)}


def pieces(emul, tmp_path, im, form):
    """dfa_resume_emul pieces: every round against the oracle on what has been given so far, the last against one piece per string"""
    strings, is_rev = im["strings"], im["info"]["is_reversed"]
    rng = np.random.default_rng(len(strings) + states(im))
    rounds = rounds_of(strings, cuts_for(strings, rng), is_rev)
    off = out_offsets(strings)
    data, poff = oracle_lib.pack(strings)
    start = [capi.DFA_STATE_START] * len(strings)
    whole_st, whole_res = run_pieces(emul, tmp_path, im["blob"], data, int(poff[-1]), start, [[(o, o + len(s)) for o, s in zip(off, strings)]], form)
    differ(whole_res[0], im, "whole strings, " + form)
    st, res = run_pieces(emul, tmp_path, im["blob"], data, int(poff[-1]), start, [[(o + b, o + e) for o, (b, e) in zip(off, row)] for row in rounds], form)
    ora = oracle_lib.OracleImage(im["blob"])
    for r in range(ROUNDS - 1):
        assert np.array_equal(res[r], ora.match(seen_so_far(strings, rounds, r, is_rev))), (im["what"], form, r)
    differ(res[-1], im, "pieces, " + form)
    assert np.array_equal(st[-1], whole_st[0]) and int(st.max()) < states(im), (im["what"], form)


@pytest.mark.parametrize("seed", SEEDS)
def test_split_and_resume_cores(seed, tmp_path):
    """up to 127 state sets: dfa_split_emul with chunks of 16 and 48 bytes, dfa_resume_emul pieces on the LDS form and fold from every
    start state; above: pieces on the L2 form"""
    split, resume = emul_exe("dfa_split"), emul_exe("dfa_resume")
    small = big = 0
    for im in nfa_fuzz.cpu_corpus(seed):
        if not states(im):
            continue
        (tmp_path / "a.blob").write_bytes(im["blob"])
        write_batch(tmp_path / "batch.bin", im["strings"])
        if states(im) > 127:
            pieces(resume, tmp_path, im, "big")
            big += 1
            continue
        for chunk, tile in ((16, 2048), (48, 512)):
            p = harness([split, tmp_path / "a.blob", tmp_path / "batch.bin", chunk, 1 << 20, tile])
            if p is not None:
                differ(np.array([int(x) for x in p.stdout.split()[2:]], dtype=np.uint8), im, "dfa_split_emul chunk %d" % chunk)
            p = harness([resume, "fold", tmp_path / "a.blob", tmp_path / "batch.bin", chunk, tile])
            assert p is None or p.stdout.split() == [b"ok", b"%d" % states(im), b"%d" % (states(im) * len(im["strings"]))], im["what"]
        pieces(resume, tmp_path, im, "lds")
        pieces(resume, tmp_path, im, "big")
        small += 1
    assert small >= 20 and big >= 4


@pytest.mark.parametrize("seed", SEEDS)
def test_spec_core(seed, tmp_path):
    """255 state sets and more: dfa_spec_emul with chunks of 16 bytes, 0 and 3 repair rounds, from {start} and (on the first 40 strings)
    from every state set"""
    emul = emul_exe("dfa_spec")
    done = 0
    for im in nfa_fuzz.cpu_corpus(seed):
        if states(im) < 255:
            continue
        (tmp_path / "a.blob").write_bytes(im["blob"])
        for rounds in (0, 3):
            write_batch(tmp_path / "batch.bin", im["strings"])
            got, res = run_spec(emul, tmp_path, 16, 16, rounds, "one")
            assert got["states"] == states(im) and got["checks"] == len(im["strings"]), im["what"]
            differ(res, im, "dfa_spec_emul, %d rounds" % rounds)
            write_batch(tmp_path / "batch.bin", im["strings"][:40])
            got, _ = run_spec(emul, tmp_path, 16, 16, rounds, "every")
            assert got["checks"] == (states(im) - 1) * 40, im["what"]
        done += 1
    assert done >= 2


def eight_alphabets(c):
    """eight images the multi-table kernel takes (up to 55 state sets) whose label sets all differ, both directions among them"""
    out = []
    for rev in (0, 1, 0, 1, 0, 1, 0, 1):
        out.append(next(im for im in c if 1 <= states(im) <= 55 and im["info"]["is_reversed"] == rev and all(im["labels"] != o["labels"] for o in out)))
    return out


@pytest.mark.parametrize("seed", SEEDS)
def test_mixed_core(seed, tmp_path):
    """dfa_mixed_emul on ONE item list of eight images with different alphabets: a table reload that kept the previous automaton's byte
    classes would show"""
    emul = emul_exe("dfa_mixed")
    eight = eight_alphabets(nfa_fuzz.cpu_corpus(seed))
    strings, items, want, blobs = [], [], [], []
    for k, im in enumerate(eight):
        (tmp_path / ("%d.blob" % k)).write_bytes(im["blob"])
        blobs.append(tmp_path / ("%d.blob" % k))
        items.append((len(strings), len(im["strings"]), k))
        strings += im["strings"]
        want += list(im["want"])
    data, off = oracle_lib.pack(strings)
    (tmp_path / "batch.bin").write_bytes(struct.pack("<QQ", len(strings), len(items)) + off.astype("<u8").tobytes()
                                         + b"".join(struct.pack("<QQQ", *i) for i in items) + data.tobytes()[:int(off[-1])])
    p = harness([emul, tmp_path / "batch.bin"] + blobs)
    assert p is not None
    got = np.array([int(x) for x in p.stdout.decode().split("\n")[1:1 + len(strings)]])
    bad = np.nonzero(got != np.array(want))[0]
    assert bad.size == 0, "%d differences, first: string %d %r want %d got %d" % (bad.size, bad[0], strings[bad[0]][:40], want[bad[0]], got[bad[0]])


@pytest.mark.parametrize("seed", SEEDS)
def test_set_resume_core(seed, tmp_path):
    """the nfa_set_resume harness on one image per mask width and direction: pieces in ROUNDS rounds against the oracle, the final
    records against those of the whole strings"""
    exe = setresume_lib.resume_emul_exe()
    c = nfa_fuzz.cpu_corpus(seed)
    for w in (1, 2, 4, 8):
        for rev in (0, 1):
            im = next(i for i in c if nfa_fuzz.mask_words(i["info"]) == w and i["info"]["is_reversed"] == rev)
            rounds, is_rev = setresume_lib.piece_rounds(im["blob"], im["strings"], np.random.default_rng(8 * w + rev))
            assert is_rev == rev
            digits, recs = setresume_lib.run_pieces(exe, tmp_path, im["blob"], im["strings"], rounds)
            ora = oracle_lib.OracleImage(im["blob"])
            for r in range(ROUNDS - 1):
                assert np.array_equal(digits[r], ora.match(seen_so_far(im["strings"], rounds, r, rev))), (im["what"], r)
            differ(digits[-1], im, "nfa_set_resume_emul pieces")
            whole_digits, whole_recs = setresume_lib.run_pieces(exe, tmp_path, im["blob"], im["strings"], setresume_lib.whole(im["strings"]))
            differ(whole_digits[0], im, "nfa_set_resume_emul whole")
            assert np.array_equal(recs, whole_recs), im["what"]
            setresume_lib.check_records_are_clean(recs, im["info"]["n_nodes"])


def test_refusals_stay_under_the_cap():
    """(runs last in this file) a harness that refused an image was not compared: at most 5 % of the runs"""
    print("harness runs: %(run)d, refused: %(refused)d" % _runs)
    assert _runs["refused"] <= nfa_fuzz.REFUSAL_CAP * max(_runs["run"], 1)
