"""Would the fuzz notice?  Faults planted in COPIES of the walk source -- the created-cell fields cm, com and rdm narrowed where ee_decode
unpacks them, a created cell never open in frame_state, an open bit or the read marks dropped where the table builder recurses -- must
each make the one-lane build (tests/emul/) disagree with the CPU restatement on at least one image of the second family's nine-cell-limit corpus of seed 0 (tests/regex_fuzz.py: it carries every
directed regex).  The unplanted copy, built the same way, must agree on all of them.

A planted tree is a temporary copy of include/ and of csrc's headers, walk_tables.cpp and image_host.cpp in the repository's layout
(the headers include ../../include/... relatively); tests/emul/build.sh compiles it through EMUL_ROOT.  A fault is ONE exact text
replacement: a text that is no longer there exactly once fails the test, and the list below is to be brought up to date."""
import glob
import os
import shutil
from concurrent.futures import ThreadPoolExecutor
import subprocess

import numpy as np
import pytest

import oracle_lib
import regex_fuzz
from testlib import CSRC, EMUL_DIR, walk_emul_run

REL_CSRC = os.path.relpath(CSRC, oracle_lib.ROOT)
CORE, TABLES = os.path.join(REL_CSRC, "walk_core.h"), os.path.join(REL_CSRC, "walk_tables.cpp")
N_REGEX, NCELL, SETTING = 44, 9, (8, 0)                     # the corpus of tests/test_walk_fuzz_cpu.py; (list capacity, regions)

# name -> (file, text, replacement)
FAULTS = {
    "cm, two-word edges: cells 4-6 lost": (CORE, "cm = (e1 >> 12) & 0x3fu", "cm = (e1 >> 12) & 0x07u"),
    "cm, three-word edges: cell 9 lost": (CORE, "cm = (e1 >> 18) & 0x1ffu", "cm = (e1 >> 18) & 0xffu"),
    "com, two-word edges: cells 4-6 lost": (CORE, "com = (e1 >> 18) & 0x3fu", "com = (e1 >> 18) & 0x07u"),
    "com, three-word edges: cell 9 lost": (CORE, "com = e2 & 0x1ffu", "com = e2 & 0xffu"),
    "rdm, two-word edges: cells 4-6 lost": (CORE, "rdm = (e1 >> 24) & 0x3fu", "rdm = (e1 >> 24) & 0x07u"),
    "rdm, three-word edges: cell 9 lost": (CORE, "rdm = (e2 >> 9) & 0x1ffu", "rdm = (e2 >> 9) & 0xffu"),
    "a created cell is never open": (CORE, "(((com >> c) & 1u) ? F_OPEN : 0u)", "0u"),
    # in the table builder.  The first is seen by the directed shape "from a waiting state", the second only by "a chain ... from a waiting
    # state" (two cells created behind one another while the state waits), the third only by the images scanned from the end by force
    # (a read of a never-set cell behind a read attempt of a set one, which no -reverse image keeps): regex_fuzz.directed_trees
    "flat_c: the waiting insertion without its own cell's open bit": (
        TABLES, "v.c.push_back(SymEdge{0u, 0u, e.target, fm2, 0u, cm2, com2, 0u});", "v.c.push_back(SymEdge{0u, 0u, e.target, fm2, 0u, cm2, com, 0u});"),
    "flat_c: the recursion without the cell's open bit": (TABLES, "flat_c(e.target, fm2, cm2, com2, false, v);", "flat_c(e.target, fm2, cm2, com, false, v);"),
    "flat_b: the recursion without the frame's read marks": (
        TABLES, "com | (open ? 1u << d : 0u), rd, cls, out);", "com | (open ? 1u << d : 0u), 0u, cls, out);"),
}
UNPLANTED = "no fault"


def plant(root, fault):
    """the copy of the walk source under `root`, with the fault's replacement made"""
    os.makedirs(os.path.join(root, REL_CSRC))
    shutil.copytree(os.path.join(oracle_lib.ROOT, "include"), os.path.join(root, "include"))
    for pattern in ("*.h", "walk_tables.cpp", "image_host.cpp"):
        for src in glob.glob(os.path.join(CSRC, pattern)):
            shutil.copy(src, os.path.join(root, REL_CSRC))
    if fault is not None:
        name, old, new = fault
        with open(os.path.join(root, name)) as f:
            text = f.read()
        assert text.count(old) == 1, "%s holds %r %d times, not once: the fault list of %s needs updating" % (name, old, text.count(old), __file__)
        with open(os.path.join(root, name), "w") as f:
            f.write(text.replace(old, new))


def build(root):
    exe = os.path.join(root, "walk_emul")
    p = subprocess.run([os.path.join(EMUL_DIR, "build.sh"), "walk", exe], env=dict(os.environ, EMUL_ROOT=root), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, "tests/emul/build.sh walk failed on %s:\n%s" % (root, p.stdout)
    return exe


def disagreeing(exe, corpus, wants, folder):
    """the images (regex, flag) on which the build's answers are not the restatement's (a build that fails on an image disagrees on it)"""
    out = []
    path = os.path.join(folder, "a.blob")
    for (regex, flag, blob, strings), want in zip(corpus, wants):
        with open(path, "wb") as f:
            f.write(blob)
        try:
            got = walk_emul_run(exe, path, SETTING[0], SETTING[1], strings)[0]
        except AssertionError:
            got = None
        if got is None or len(got) != len(want) or (got != want).any():
            out.append((regex, flag))
    return out


_found = None


def found(tmp):
    """name -> the images that disagree, for the unplanted copy and every fault: planted, built (eight compilers at a time) and walked once"""
    global _found
    if _found is None:
        corpus = regex_fuzz.corpus(0, N_REGEX, NCELL, family=2)
        wants = [np.asarray(oracle_lib.OracleImage(blob).match(strings)).copy() for regex, flag, blob, strings in corpus]
        names = [UNPLANTED] + list(FAULTS)
        roots = [str(tmp / ("tree%d" % k)) for k in range(len(names))]
        for name, root in zip(names, roots):
            plant(root, FAULTS.get(name))

        def one(root):
            return disagreeing(build(root), corpus, wants, root)

        with ThreadPoolExecutor(max_workers=8) as pool:
            _found = dict(zip(names, pool.map(one, roots)))
        for name in names:
            print("%-40s %3d of %d images disagree%s" % (name, len(_found[name]), len(corpus), ", first %r %s" % _found[name][0] if _found[name] else ""))
    return _found


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    return found(tmp_path_factory.mktemp("planted"))


def test_the_unplanted_copy_agrees(results):
    assert results[UNPLANTED] == []


@pytest.mark.parametrize("name", list(FAULTS))
def test_planted_fault_is_caught(results, name):
    assert len(results[name]) >= 1, "no image of the corpus notices: %s" % name
