"""Random regexes through the host front-end against the reference itself (needs oracle/_ref/ref_harness, i.e. the
build container; skipped elsewhere): the automaton images must be identical, node order and edge order included."""
import os
import random
import subprocess

import pytest

import oracle_lib
from testlib import DIPLOMA, rand_regex

HARNESS = os.path.join(oracle_lib.ROOT, "oracle", "_ref", "ref_harness")

pytestmark = pytest.mark.skipif(not (os.path.exists(HARNESS) and os.path.exists(DIPLOMA)),
                                reason="needs the reference harness (build container only)")


def dump_pair(regex, flag, mode, tmp):
    a = subprocess.run([DIPLOMA, "-dump"] + flag, input=regex + "\n", capture_output=True, text=True, cwd=tmp)
    b = subprocess.run([HARNESS, "dump", mode, regex], capture_output=True, text=True, cwd=tmp)
    return a, b


@pytest.mark.parametrize("seed", range(6))
def test_random_regexes_match_reference(seed, tmp_path):
    rng = random.Random(1000 + seed)
    checked = 0
    for _ in range(40):
        mem = rng.random() < 0.6
        regex = rand_regex(rng, rng.randint(1, 3), [], mem)
        if len(regex) < 2:
            continue
        if mem and ("{" in regex or "&" in regex):
            modes = [(["-mfa"], "mfa"), ([], "plain")]
        else:
            modes = [(["-thompson"], "thompson"), (["-glushkov"], "glushkov"), ([], "plain")]
        for flag, mode in modes:
            a, b = dump_pair(regex, flag, mode, tmp_path)
            if b.returncode != 0 or "UNKNOWN" in b.stdout:
                continue                      # the reference itself cannot build this one
            assert a.returncode == 0, (regex, mode, a.stderr)
            assert a.stdout == b.stdout, "regex %r mode %s" % (regex, mode)
            checked += 1
    assert checked > 40


def rand_memory_regex(rng, depth, cells):
    """random regexes with nested initialisations, reads inside initialisations and up to three cells: what the BNF rewriter's
    distribute / open-Kleene / denesting / sliding steps key on"""
    if depth <= 0:
        if cells and rng.random() < 0.35:
            return "&" + rng.choice(cells)
        return rng.choice("abc")
    kind = rng.random()
    if kind < 0.35:
        return "".join(rand_memory_regex(rng, depth - 1, cells) for _ in range(rng.randint(2, 3)))
    if kind < 0.55:
        return "(" + "|".join(rand_memory_regex(rng, depth - 1, cells) for _ in range(rng.randint(2, 3))) + ")"
    if kind < 0.72:
        return "(" + rand_memory_regex(rng, depth - 1, cells) + ")*"
    if kind < 0.92:
        k = rng.choice("123")
        inner = rand_memory_regex(rng, depth - 1, [c for c in cells if c != k])
        if k not in cells:
            cells.append(k)
        return "{" + inner + "}:" + k
    return rng.choice("abc") + "*"


@pytest.mark.parametrize("seed", range(4))
def test_bnf_and_reverse_match_reference(seed, tmp_path):
    """The rewritten regexes as strings (the reference's REPL) and the automata `-bnf` / `-reverse` build from them, against
    the reference on random regexes.  Cases on which the reference itself dies (null dereferences in its rewriter) are skipped;
    on everything it survives this build must give the same and must not throw."""
    rng = random.Random(7000 + seed)
    strings_ok = images_ok = 0
    for _ in range(120):
        regex = rand_memory_regex(rng, rng.randint(1, 4), [])
        if "{" not in regex and "&" not in regex:
            continue
        try:
            b = subprocess.run([HARNESS, "front", regex], capture_output=True, text=True, cwd=tmp_path, timeout=20)
        except subprocess.TimeoutExpired:
            continue
        if b.returncode != 0:
            continue
        a = subprocess.run([DIPLOMA], input=regex + "\nexit\n", capture_output=True, text=True, cwd=tmp_path, timeout=20)
        assert a.returncode == 0, (regex, a.stderr)
        want = "\n".join(ln for ln in b.stdout.split("\n") if ln != "BAD")       # the harness's own marker for is_bad_bnf
        assert a.stdout == want, "regex %r" % regex
        strings_ok += 1
        for flag, mode in ((["-bnf"], "bnf"), (["-reverse"], "reverse")):
            try:
                d = subprocess.run([HARNESS, "dump", mode, regex], capture_output=True, text=True, cwd=tmp_path, timeout=20)
            except subprocess.TimeoutExpired:
                continue
            if d.returncode != 0 or "UNKNOWN" in d.stdout:
                continue
            m = subprocess.run([DIPLOMA, "-dump"] + flag, input=regex + "\n", capture_output=True, text=True, cwd=tmp_path, timeout=20)
            assert m.returncode == 0, (regex, mode, m.stderr)
            assert m.stdout == d.stdout, "regex %r mode %s" % (regex, mode)
            images_ok += 1
    assert strings_ok > 40 and images_ok > 60


@pytest.mark.parametrize("seed", range(4))
def test_restatement_on_random_regexes(seed, tmp_path):
    """The CPU restatement against the reference on automata and strings outside the committed fixtures."""
    import numpy as np
    from mfa_amd import image
    rng = random.Random(5000 + seed)
    done = 0
    for _ in range(30):
        if done >= 8:
            break
        regex = rand_regex(rng, rng.randint(2, 3), [], True)
        if "{" not in regex and "&" not in regex:
            continue
        d = subprocess.run([HARNESS, "dump", "mfa", regex], capture_output=True, text=True, cwd=tmp_path)
        if d.returncode != 0 or "UNKNOWN" in d.stdout:
            continue
        try:
            blob = image.blob_from_dump(d.stdout)
        except image.ImageError:
            continue
        strings = []
        for _k in range(150):
            n = rng.randint(0, 40)
            strings.append("".join(rng.choice("aaabbc") for _ in range(n)))
        for _k in range(30):
            w = "".join(rng.choice("ab") for _ in range(rng.randint(1, 3)))
            strings.append(w * rng.randint(1, 30) + rng.choice(["", "a", "b", "c"]))
        strings = [s for s in strings if s]                       # the harness reads lines; keep it simple
        r = subprocess.run([HARNESS, "match", "mfa", regex], input="".join(s + "\n" for s in strings), capture_output=True, text=True,
                           cwd=tmp_path)
        assert r.returncode == 0
        want = np.array([int(c) for c in r.stdout.split()], dtype=np.uint8)
        got = oracle_lib.OracleImage(blob).match([s.encode() for s in strings])
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, "regex %r: %d mismatches, first %r want %d" % (regex, bad.size, strings[bad[0]], want[bad[0]])
        done += 1
    assert done >= 4
