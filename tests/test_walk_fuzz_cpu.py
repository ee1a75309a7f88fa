"""The walk kernel's source as a wave of one lane (tests/emul/, as in test_walk_emul.py) on automata nobody has seen before: random
regexes of up to nine cells through the host front-end as -mfa, -bnf and -reverse images, on strings sampled from the regex itself
(tests/regex_fuzz.py: accepted strings and near misses, star bodies pumped up to 1 000 times), against the CPU restatement.  What a corpus
must exercise -- both answers, jumps, spills, every cell count -- is asserted, not hoped for.  MFA_FUZZ_SEEDS=n: n more seeds per cell limit
(MFA_FUZZ_FIRST=k: seeds k .. k + n).

Two families of regexes.  The first never reads a cell before it is set.  The second does (regex_fuzz.gen_tree2, directed_trees): a read
of an absent cell creates it, and {&k r}:k creates it OPEN -- the table fields cm, com and rdm of every effective edge (walk_tables.h),
unpacked by ee_decode and applied by frame_state.  For the second family the coverage is asserted per cell and per edge width, in the
tables (walk_emul's EMUL_FIELDS counts) and in the restatement's own run (mfa_oracle_stats: created_open, mark_decided)."""
import hashlib
import os

import numpy as np
import pytest

import oracle_lib
import regex_fuzz
from mfa_amd import image
from testlib import emul_exe, walk_emul_run as emul_run

HARNESS = os.path.join(oracle_lib.ROOT, "oracle", "_ref", "ref_harness")
N_REGEX = 44
RUNS = ((8, 0), (2, 0), (8, 1), (3, 1))        # (list capacity, regions)
MAP_RUNS = ((2, 0), (3, 1))
FIELDS = ("c-cm", "c-com", "c-rdm", "b-cm", "b-com", "b-rdm")

_first = int(os.environ.get("MFA_FUZZ_FIRST", "0"))
_seeds = range(_first, _first + 1 + int(os.environ.get("MFA_FUZZ_SEEDS", "0")))
SEEDS = [(seed, ncell) for seed in _seeds for ncell in (3, 6, 9)]

_corpora = {}
_wants = {}


@pytest.fixture(scope="module")
def emul():
    return emul_exe("walk")


@pytest.fixture(scope="module")
def emul_map():
    return emul_exe("walk", "-DWALK_NODE_MAP=1")


def corpus_of(seed, ncell, family=1):
    if (seed, ncell, family) not in _corpora:
        _corpora[(seed, ncell, family)] = regex_fuzz.corpus(seed, N_REGEX, ncell, family=family)
    return _corpora[(seed, ncell, family)]


def wants_of(seed, ncell, family=1):
    """[(the restatement's answers, its counters)] image by image, computed once"""
    if (seed, ncell, family) not in _wants:
        out = []
        for regex, flag, blob, strings in corpus_of(seed, ncell, family):
            stats = oracle_lib.Stats()
            want = np.asarray(oracle_lib.OracleImage(blob).match(strings, stats)).copy()
            want.setflags(write=False)
            out.append((want, stats))
        _wants[(seed, ncell, family)] = out
    return _wants[(seed, ncell, family)]


def check(got, want, regex, flag, cap, accel, strings, build=""):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "regex %r %s%s capacity %d regions %d: %d of %d strings wrong, first %r (len %d) want %d got %d" % (
        regex, flag, build, cap, accel, bad.size, len(strings), strings[bad[0]][:80], len(strings[bad[0]]), want[bad[0]], got[bad[0]])


def walk_corpus(emul, emul_map, seed, ncell, family, path):
    """every image at the four settings (one-cell images through the node-map build too); what a corpus must exercise, asserted"""
    walked = both = jumped = spilled = 0
    cell_counts = set()
    for (regex, flag, blob, strings), (want, _) in zip(corpus_of(seed, ncell, family), wants_of(seed, ncell, family)):
        path.write_bytes(blob)
        for cap, accel in RUNS:
            got, stats = emul_run(emul, path, cap, accel, strings)
            check(got, want, regex, flag, cap, accel, strings)
            if (cap, accel) == (8, 1):
                jumped += stats["hits"] > 0
            if (cap, accel) == (3, 1):
                spilled += stats["spill-steps"] > 0
        cells = image.blob_info(blob)["n_cells"]
        if cells == 1:                                      # the long-list kernel's form of the insertion: one-cell automata only
            for cap, accel in MAP_RUNS:
                got, _ = emul_run(emul_map, path, cap, accel, strings)
                check(got, want, regex, flag, cap, accel, strings, " (node map)")
        walked += 1
        both += 0.1 <= want.mean() <= 0.9
        cell_counts.add(cells)
    print("family %d seed %d ncell %d: %d images, both answers %d, jumps %d, spills %d, cell counts %s" % (
        family, seed, ncell, walked, both, jumped, spilled, sorted(cell_counts)))
    assert walked >= 100
    assert both >= 0.6 * walked
    assert jumped >= 0.5 * walked
    assert spilled >= 0.1 * walked
    if ncell == 9:
        assert cell_counts >= set(range(1, 10)), sorted(cell_counts)


@pytest.mark.parametrize("seed,ncell", SEEDS)
def test_walk_source_on_random_automata(emul, emul_map, seed, ncell, tmp_path):
    walk_corpus(emul, emul_map, seed, ncell, 1, tmp_path / "a.blob")


# ---- the second family: cells created by a read ---------------------------------------------------------------------------------------------
def corpus_digest(corpus):
    h = hashlib.sha256()
    for regex, flag, blob, strings in corpus:
        for part in [regex.encode(), flag.encode(), blob] + list(strings):
            h.update(len(part).to_bytes(4, "little"))
            h.update(part)
    return len(corpus), h.hexdigest()


def test_the_first_family_is_what_it_was():
    """corpus(..., family=1) image for image (regex, flag, blob, strings) as before the second family came: the GPU tests' first corpus
    and the build's list of kernels to compile ahead are cut from it"""
    was = {3: (114, "4422b30b42694bfc18cb30f575ef3c60f9959fd279884ca4366dd356214fec18"),
           6: (120, "53ab2b85ac9201c55cffd4bc136ff27040b819bc3324b7bd95b36f7d662ac2a7"),
           9: (126, "0c4b25b39c9d899065a981b03fb2412f986d82db47df497140600c7991935f38")}
    for ncell in (3, 6, 9):
        assert corpus_digest(regex_fuzz.corpus(0, N_REGEX, ncell)) == was[ncell], ncell
    gpu = regex_fuzz.corpus(regex_fuzz.GPU_SEED, regex_fuzz.GPU_REGEXES, regex_fuzz.GPU_NCELL, regex_fuzz.GPU_SAMPLES)
    assert corpus_digest(gpu) == (235, "f72b6170fa75b7add558bb05f2541593b8c5871d16f3122a7a55001c82e49f66")


def wide_partner(seed, rev):
    """(blob, a few strings, their answers) of the first directed nine-cell -mfa or -reverse image of the seed that scans in direction rev"""
    corpus = corpus_of(seed, 9, 2)
    for k in range(corpus.first_directed, len(corpus)):
        regex, flag, blob, strings = corpus[k]
        info = image.blob_info(blob)
        if info["n_cells"] == 9 and info["reversed"] == rev and flag != "-bnf":
            return blob, strings[:7], wants_of(seed, 9, 2)[k][0][:7]
    raise AssertionError("no directed nine-cell image with reversed == %d" % rev)


@pytest.mark.parametrize("seed,ncell", SEEDS)
def test_walk_source_on_created_cells(emul, emul_map, seed, ncell, tmp_path):
    walk_corpus(emul, emul_map, seed, ncell, 2, tmp_path / "a.blob")
    # every directed image of at most six cells once more, as the first segment of a launch whose second automaton has nine cells: its
    # tables then have three-word edges and the step is the K = 9 instantiation ("the field positions do not depend on the automaton's
    # own cell count", walk_tables.h)
    corpus, wants = corpus_of(seed, ncell, 2), wants_of(seed, ncell, 2)
    first, second, again = tmp_path / "first.blob", tmp_path / "second.blob", 0
    for k in range(corpus.first_directed, len(corpus)):
        regex, flag, blob, strings = corpus[k]
        info = image.blob_info(blob)
        if info["n_cells"] > 6:
            continue
        wide, more, more_want = wide_partner(seed, info["reversed"])
        first.write_bytes(blob)
        second.write_bytes(wide)
        got, stats = emul_run(emul, first, 3, 1, strings + more, more=[second, len(strings)])
        check(got, np.concatenate([wants[k][0], more_want]), regex, flag, 3, 1, strings + more, " (beside a nine-cell automaton)")
        assert stats["fields"] == regex_fuzz.table_fields(blob), (regex, flag)
        again += 1
    assert again >= 3 * min(ncell, 6)


@pytest.mark.parametrize("seed", list(_seeds))
def test_created_cells_are_covered(emul, seed, tmp_path):
    """Over the three second-family corpora of a seed.  In the TABLES: for every cell 1..6 among the images of at most six cells (two-word
    edges), and for every cell 1..9 among the images of seven to nine cells (three-word edges), at least three images hold the cell in cm,
    three in com, and three images with reversed == 1 in rdm.  In the RESTATEMENT's run on the corpora's strings: every cell is created
    open, and in reversed images of both widths an is_read mark decides a suffix check."""
    path = tmp_path / "a.blob"
    held = {(wide, f): [0] * 9 for wide in (False, True) for f in ("cm", "com", "rdm", "c-com", "b-com")}
    created_open, decided = [0] * 10, {False: 0, True: 0}
    for ncell in (3, 6, 9):
        for (regex, flag, blob, strings), (want, st) in zip(corpus_of(seed, ncell, 2), wants_of(seed, ncell, 2)):
            info = image.blob_info(blob)
            path.write_bytes(blob)
            fields = emul_run(emul, path, 8, 0, [])[1]["fields"]
            assert set(fields) == set(FIELDS) and fields == regex_fuzz.table_fields(blob), (regex, flag)
            wide = info["n_cells"] > 6
            for c in range(9):
                held[(wide, "cm")][c] += fields["c-cm"][c] + fields["b-cm"][c] > 0
                held[(wide, "com")][c] += fields["c-com"][c] + fields["b-com"][c] > 0
                held[(wide, "c-com")][c] += fields["c-com"][c] > 0
                held[(wide, "b-com")][c] += fields["b-com"][c] > 0
                held[(wide, "rdm")][c] += info["reversed"] == 1 and fields["b-rdm"][c] > 0
            for c in range(1, 10):
                created_open[c] += st.created_open[c]
            if info["reversed"] == 1:
                decided[wide] += st.mark_decided
    for (wide, f), n in sorted(held.items()):
        print("seed %d, images of %s cells that hold the cell in %-5s: %s" % (seed, "7-9" if wide else "1-6", f, n))
    print("seed %d, created open by cell: %s, suffix checks decided by a read mark: narrow %d wide %d" % (seed, created_open[1:], decided[False], decided[True]))
    for f in ("cm", "com", "rdm"):
        assert min(held[(False, f)][:6]) >= 3, (f, held[(False, f)])
        assert min(held[(True, f)]) >= 3, (f, held[(True, f)])
    assert min(created_open[1:]) > 0, created_open
    assert decided[False] > 0 and decided[True] > 0, decided


@pytest.mark.skipif(not (os.path.exists(HARNESS) and os.path.exists(regex_fuzz.DIPLOMA)), reason="needs the reference harness (build container only)")
def test_sampled_strings_against_the_reference(tmp_path):
    """The restatement's answers on the sampler's strings against the reference itself (20 forward images, strings of at most 400 bytes:
    the reference is slow): what the other tests of this file and the GPU fuzz compare with is tied to the reference on THESE strings too.
    Then 20 forward images of the second family that hold '{&' (strings of at most 300 bytes): cells created open, in the reference."""
    import subprocess
    for family, longest in ((1, 400), (2, 300)):
        images = [c for c in corpus_of(SEEDS[0][0], 9, family) if c[1] == "-mfa" and (family == 1 or "{&" in c[0])]
        done = 0
        for regex, flag, blob, strings in images[::max(1, len(images) // 20)][:20]:
            short = [s for s in strings if len(s) <= longest]
            r = subprocess.run([HARNESS, "match", "mfa", regex], input=b"".join(s + b"\n" for s in short), capture_output=True, cwd=tmp_path)
            assert r.returncode == 0, (regex, r.stderr[-300:])
            want = np.array([int(c) for c in r.stdout.split()], dtype=np.uint8)
            got = oracle_lib.OracleImage(blob).match(short)
            assert len(want) == len(short), regex
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, "regex %r: %d mismatches, first %r reference %d restatement %d" % (regex, bad.size, short[bad[0]], want[bad[0]], got[bad[0]])
            done += 1
        assert done == 20
