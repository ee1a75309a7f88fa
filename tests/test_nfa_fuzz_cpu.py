"""The memory-less engines' host-compilable cores on automata nobody has seen before (tests/nfa_fuzz.py: raw random automata with up to 200
byte classes, labels of 0x80 and above, letter edges to lower ranks, and random regexes through every compile of the host front-end), all
against the CPU restatement: the reference's step restated in Python, the set walk's mask step against the table from every state set and
class, the split path, the resume call's pieces and folds, the L2 table's guesses, the multi-table item walk and the set walk's records,
and on every image of nfa_fuzz.set_corpus the set walk's split path from {start} and from every tabulated set and the wave kernels' cores.
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
import setwalk_lib
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
    exe = emul_exe("nfa_set_resume")
    c = nfa_fuzz.cpu_corpus(seed)
    for w in (1, 2, 4, 8):
        for rev in (0, 1):
            im = next(i for i in c if nfa_fuzz.mask_words(i["info"]) == w and i["info"]["is_reversed"] == rev)
            rounds, is_rev = setwalk_lib.piece_rounds(im["blob"], im["strings"], np.random.default_rng(8 * w + rev))
            assert is_rev == rev
            digits, recs = setwalk_lib.run_lane_pieces(exe, tmp_path, im["blob"], im["strings"], rounds)
            ora = oracle_lib.OracleImage(im["blob"])
            for r in range(ROUNDS - 1):
                assert np.array_equal(digits[r], ora.match(seen_so_far(im["strings"], rounds, r, rev))), (im["what"], r)
            differ(digits[-1], im, "nfa_set_resume_emul pieces")
            whole_digits, whole_recs = setwalk_lib.run_lane_pieces(exe, tmp_path, im["blob"], im["strings"], setwalk_lib.whole(im["strings"]))
            differ(whole_digits[0], im, "nfa_set_resume_emul whole")
            assert np.array_equal(recs, whole_recs), im["what"]
            setwalk_lib.check_records_are_clean(recs, im["info"]["n_nodes"], setwalk_lib.LANE_WORDS)


# ---- the set walk's split, resume and wave cores: every image of the set corpus -------------------------------------------------------------
SPLIT_CHUNKS, SPLIT_LOOKBACKS, SPLIT_ROUNDS = (16, 48), (0, 8, 64), (0, 1, 3)


@pytest.mark.parametrize("seed", SEEDS)
def test_the_set_corpus_is_what_the_tests_count_on(seed):
    c = nfa_fuzz.set_corpus(seed)
    nfa_fuzz.report_set(c, seed)
    nfa_fuzz.check_set_lines(c)
    base = nfa_fuzz.cpu_corpus(seed)
    assert len(c) > len(base) and all(a is b for a, b in zip(c, base)) and all("twin_of" in im for im in c[len(base):])


@pytest.mark.parametrize("seed", SEEDS)
def test_set_split_core(seed, tmp_path):
    """nfa_set_split_emul from {start} on every image of the set corpus, every string cut, in all 18 combinations of chunks of 16 and 48
    bytes, lookbacks of 0, 8 and 64 bytes and 0, 1 and 3 repair rounds: the harness holds every final record to the whole walk's, word
    for word, and its result digits are the oracle's.  Random automata converge late, never, or at once, so at (16, 64, 3) at least a
    third of the images have chunks walked again, a third have strings resolved serially and a third have chunks whose guess fell back
    to the home set; without a byte of lookback or a repair, at either chunk size, every image has strings resolved serially -- but one
    whose table has two state sets, the empty set and {start}: its only live set is {start}, which no guess can miss (seed 3 draws one:
    two nodes, an epsilon edge from the start and one letter edge back to it).
    Measured, each seed 36 images (34 and the direction twins of those beyond LDS), images with chunks walked again / strings resolved
    serially / home guesses at (16, 64, 3): seed 0: 31, 29, 28; seed 1: 27, 25, 30; seed 2: 28, 24, 25; seed 3: 28, 25, 27.  Tables beyond LDS, in words: seed 0: 30 237 (W 4, 119 classes) and 188 546 (W 8, 201
    classes); seed 1: 29 699 and 190 144; seed 2: 38 123 and 186 916; seed 3: 172 437.  No run refused."""
    emul = emul_exe("nfa_set_split")
    c = nfa_fuzz.set_corpus(seed)
    done = rewalked = serial = home = 0
    for im in c:
        runs = setwalk_lib.run_lane_split(emul, tmp_path, im["blob"], im["strings"], SPLIT_CHUNKS, SPLIT_LOOKBACKS, SPLIT_ROUNDS, run=harness)
        if runs is None:
            continue
        done += 1
        assert len(runs) == 18
        for combo, counts, digits in runs:
            assert counts["W"] == nfa_fuzz.mask_words(im["info"]) and counts["checks"] == len(im["strings"]), (im["what"], combo)
            differ(digits, im, "nfa_set_split_emul one, chunk %d lookback %d rounds %d" % combo)
            if combo == (16, 64, 3):
                rewalked += counts["rewalked"] > 0
                serial += counts["serial_strings"] > 0
                home += counts["home_guesses"] > 0
            if combo[1:] == (0, 0):
                assert (counts["serial_strings"] > 0 or states(im) == 2) and counts["rewalked"] == 0, (im["what"], combo, counts)
    print("nfa_set_split_emul seed %d: %d images of %d; at (16, 64, 3) %d with chunks walked again, %d with strings resolved serially, %d with home guesses"
          % (seed, done, len(c), rewalked, serial, home))
    assert 3 * rewalked >= len(c) and 3 * serial >= len(c) and 3 * home >= len(c)


@pytest.mark.parametrize("seed", SEEDS)
def test_set_split_core_from_every_set(seed, tmp_path):
    """the resume form: nfa_set_split_emul `every` on the images of 2 to 60 state sets -- every string from {start}, from every tabulated
    node set and from the empty set, every final record held to the whole walk's from the same set -- at (16, 64, 3) and (48, 0, 0).
    Measured: seed 0, 24 images and 69 233 records per setting; seed 1, 24 and 59 153; seed 2, 25 and 72 500; seed 3, 22 and 37 950."""
    emul = emul_exe("nfa_set_split")
    done = checks = 0
    for im in nfa_fuzz.set_corpus(seed):
        if not 2 <= states(im) <= 60:
            continue
        for combo in ((16, 64, 3), (48, 0, 0)):
            runs = setwalk_lib.run_lane_split(emul, tmp_path, im["blob"], im["strings"], combo[:1], combo[1:2], combo[2:], mode="every", run=harness)
            if runs is None:
                continue
            (_, counts, digits), = runs
            assert counts["checks"] == (states(im) + 1) * len(im["strings"]), im["what"]      # {start}, and the table's sets with the empty one
            differ(digits, im, "nfa_set_split_emul every, chunk %d lookback %d rounds %d" % combo)
            checks += counts["checks"] if combo[0] == 16 else 0
        done += 1
    print("nfa_set_split_emul every, seed %d: %d images, %d records per setting" % (seed, done, checks))
    assert done >= 10


@pytest.mark.parametrize("seed", SEEDS)
def test_set_wave_cores(seed, tmp_path):
    """the wave kernels' cores on images they were not made for -- up to 200 byte classes, labels of 0x80 and above, 2 to 130 nodes:
    nfa_set_wave_emul match on every image of the set corpus, nfa_set_wave_split_emul (every string cut, every record held to the whole
    walk's) at (16, 64, 3) and (48, 0, 0), all against the oracle.  Measured: seeds 0 to 3, 36 images each, none refused."""
    wave, split = emul_exe("nfa_set_wave"), emul_exe("nfa_set_wave_split")
    done = 0
    for im in nfa_fuzz.set_corpus(seed):
        got = setwalk_lib.run_match(wave, tmp_path, im["blob"], im["strings"], run=harness)
        if got is not None:
            differ(got, im, "nfa_set_wave_emul match")
            done += 1
        for combo in ((16, 64, 3), (48, 0, 0)):
            runs = setwalk_lib.run_wave_split(split, tmp_path, im["blob"], im["strings"], combo[:1], combo[1:2], combo[2:], run=harness)
            if runs is not None:
                (_, counts, digits), = runs
                assert counts["checks"] == len(im["strings"]) and counts["W"] == setwalk_lib.words_of(im["info"]["n_nodes"]), (im["what"], combo, counts)
                differ(digits, im, "nfa_set_wave_split_emul, chunk %d lookback %d rounds %d" % combo)
    print("wave harnesses seed %d: %d images" % (seed, done))


def test_refusals_stay_under_the_cap():
    """(runs last in this file) a harness that refused an image was not compared: at most 5 % of the runs"""
    print("harness runs: %(run)d, refused: %(refused)d" % _runs)
    assert _runs["refused"] <= nfa_fuzz.REFUSAL_CAP * max(_runs["run"], 1)
