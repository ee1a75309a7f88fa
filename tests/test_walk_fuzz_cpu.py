"""The walk kernel's source as a wave of one lane (tests/emul/, as in test_walk_emul.py) on automata nobody has seen before: random
regexes of up to nine cells through the host front-end as -mfa, -bnf and -reverse images, on strings sampled from the regex itself
(tests/regex_fuzz.py: accepted strings and near misses, star bodies pumped up to 1 000 times), against the CPU restatement.  What a corpus
must exercise -- both answers, jumps, spills, every cell count -- is asserted, not hoped for.  MFA_FUZZ_SEEDS=n: n more seeds per cell limit
(MFA_FUZZ_FIRST=k: seeds k .. k + n)."""
import os
import re

import numpy as np
import pytest

import oracle_lib
import regex_fuzz
from mfa_amd import image
from testlib import emul_exe

HARNESS = os.path.join(oracle_lib.ROOT, "oracle", "_ref", "ref_harness")
N_REGEX = 44
RUNS = ((8, 0), (2, 0), (8, 1), (3, 1))        # (list capacity, regions)
MAP_RUNS = ((2, 0), (3, 1))

_first = int(os.environ.get("MFA_FUZZ_FIRST", "0"))
SEEDS = [(seed, ncell) for seed in range(_first, _first + 1 + int(os.environ.get("MFA_FUZZ_SEEDS", "0"))) for ncell in (3, 6, 9)]

_corpora = {}


@pytest.fixture(scope="module")
def emul():
    return emul_exe("walk")


@pytest.fixture(scope="module")
def emul_map():
    return emul_exe("walk", "-DWALK_NODE_MAP=1")


def corpus_of(seed, ncell):
    if (seed, ncell) not in _corpora:
        _corpora[(seed, ncell)] = regex_fuzz.corpus(seed, N_REGEX, ncell)
    return _corpora[(seed, ncell)]


def emul_run(exe, path, cap, accel, strings):
    """(answers, the counters of the emulation's last stderr line)"""
    import subprocess
    p = subprocess.run([exe, str(path), str(cap), str(accel)], input=b"".join(s + b"\n" for s in strings), capture_output=True)
    assert p.returncode == 0, p.stderr.decode()[-400:]
    line = p.stderr.decode().strip().split("\n")[-1]
    stats = {k: int(v) for k, v in re.findall(r"([a-z-]+) (\d+)", line.split("strings,")[1])}
    return np.array([int(x) for x in p.stdout.split()], dtype=np.uint8), stats


def check(got, want, regex, flag, cap, accel, strings, build=""):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "regex %r %s%s capacity %d regions %d: %d of %d strings wrong, first %r (len %d) want %d got %d" % (
        regex, flag, build, cap, accel, bad.size, len(strings), strings[bad[0]][:80], len(strings[bad[0]]), want[bad[0]], got[bad[0]])


@pytest.mark.parametrize("seed,ncell", SEEDS)
def test_walk_source_on_random_automata(emul, emul_map, seed, ncell, tmp_path):
    walked = both = jumped = spilled = 0
    cell_counts = set()
    path = tmp_path / "a.blob"
    for regex, flag, blob, strings in corpus_of(seed, ncell):
        want = oracle_lib.OracleImage(blob).match(strings)
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
    print("seed %d ncell %d: %d images, both answers %d, jumps %d, spills %d, cell counts %s" % (seed, ncell, walked, both, jumped, spilled, sorted(cell_counts)))
    assert walked >= 100
    assert both >= 0.6 * walked
    assert jumped >= 0.5 * walked
    assert spilled >= 0.1 * walked
    if ncell == 9:
        assert cell_counts >= set(range(1, 10)), sorted(cell_counts)


@pytest.mark.skipif(not (os.path.exists(HARNESS) and os.path.exists(regex_fuzz.DIPLOMA)), reason="needs the reference harness (build container only)")
def test_sampled_strings_against_the_reference(tmp_path):
    """The restatement's answers on the sampler's strings against the reference itself (20 forward images, strings of at most 400 bytes:
    the reference is slow): what the other tests of this file and the GPU fuzz compare with is tied to the reference on THESE strings too."""
    import subprocess
    images = [c for c in corpus_of(SEEDS[0][0], 9) if c[1] == "-mfa"]
    done = 0
    for regex, flag, blob, strings in images[::max(1, len(images) // 20)][:20]:
        short = [s for s in strings if len(s) <= 400]
        r = subprocess.run([HARNESS, "match", "mfa", regex], input=b"".join(s + b"\n" for s in short), capture_output=True, cwd=tmp_path)
        assert r.returncode == 0, (regex, r.stderr[-300:])
        want = np.array([int(c) for c in r.stdout.split()], dtype=np.uint8)
        got = oracle_lib.OracleImage(blob).match(short)
        assert len(want) == len(short), regex
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, "regex %r: %d mismatches, first %r reference %d restatement %d" % (regex, bad.size, short[bad[0]], want[bad[0]], got[bad[0]])
        done += 1
    assert done == 20
