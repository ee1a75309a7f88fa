"""Both walk engines on automata nobody has seen before, on the GPU: what the one-lane host build of the walk source
(tests/test_walk_fuzz_cpu.py) cannot see -- 64 lanes with different strings, 64 lanes with different AUTOMATA, per-wave spill areas, the
ticket dispenser, the lean queue, and the generated kernel, which has no host build at all.

One fixed corpus (tests/regex_fuzz.py: gpu_corpus, seed 0): 24 images of random regexes of up to nine cells -- forward, -bnf and -reverse --
each with about 330 strings sampled from its regex.  Every batch is shuffled, has a length that is no multiple of 64, is uploaded with exactly
the room the 16-byte read rule asks for, and is answered into a buffer prefilled with 7 with 64 guard bytes behind it.

A second fixed corpus (gpu_corpus2, seed 0 of the second family): 16 images whose tables hold cells CREATED by a read -- created open (com),
in byte-class and in waiting lists, with two- and with three-word edges -- and read marks of a reversed scan (rdm): the fields the CPU
fuzz covers cell by cell (tests/test_walk_fuzz_cpu.py), here with 64 lanes of different automata in a wave and in the generated kernel,
which applies them in code of its own (jit_gen.cpp: unset_cell, the phase-C insertion)."""
import numpy as np
import pytest

import oracle_lib
import regex_fuzz
import testlib
from mfa_amd import capi, image

pytestmark = pytest.mark.gpu

GUARD = 64
_want = {}


def corpus(which=1):
    return regex_fuzz.gpu_corpus() if which == 1 else regex_fuzz.gpu_corpus2()


def want_of(k, which=1):
    """the restatement's answers for image k's batch, computed once"""
    if (k, which) not in _want:
        im = corpus(which)[k]
        _want[(k, which)] = np.asarray(oracle_lib.OracleImage(im["blob"]).match(im["strings"])).copy()
        _want[(k, which)].setflags(write=False)
    return _want[(k, which)]


def upload(strings):
    """with exactly the room the read rule asks for behind the strings"""
    return testlib.upload(strings, exact=True)[:2]


def guarded(n):
    import torch
    return torch.full((n + GUARD,), 7, dtype=torch.uint8, device="cuda")


def answers(buf, n, what):
    """the n answers of a guarded buffer; the guard bytes must be untouched"""
    import torch
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[n:] == 7).all(), "%s: bytes behind the results were written" % (what,)
    return host[:n]


def compare(got, want, strings, what):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s: %d of %d strings wrong, first %r (len %d) want %d got %d" % (
        what, bad.size, len(strings), strings[bad[0]][:80], len(strings[bad[0]]), want[bad[0]], got[bad[0]])


def set_env(monkeypatch, env):
    for name in ("MFA_WALK_C", "MFA_WALK_IMAGES_GLOBAL", "MFA_WALK_TABLES_GLOBAL", "MFA_WALK_REFILL", "MFA_ACCEL", "MFA_WALK_LEAN", "MFA_MIXED_CUTS"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def test_the_corpus_is_what_the_tests_count_on():
    c = corpus()
    assert len(c) == 24
    assert all(im["flag"] == "-mfa" and 1 <= im["cells"] <= 3 for im in c[:8])
    assert all(im["flag"] == "-mfa" and 4 <= im["cells"] <= 9 for im in c[8:12]) and c[11]["cells"] >= 7
    assert all(im["flag"] == "-bnf" for im in c[12:18]) and all(im["flag"] == "-reverse" for im in c[18:])
    assert all(image.blob_info(im["blob"])["reversed"] == (1 if im["flag"] == "-reverse" else 0) for im in c)
    for k, im in enumerate(c):
        n = len(im["strings"])
        assert 165 <= n <= 330 and n % 64 != 0 and sum(len(s) for s in im["strings"]) < 1 << 20
    # both answers on 10-90 % of the strings, in at least 60 % of the batches (what tests/test_walk_fuzz_cpu.py asks of its corpora)
    assert sum(0.1 <= want_of(k).mean() <= 0.9 for k in range(24)) >= 0.6 * 24


# ---- a. one image, the table engine, under every development knob that changes where lists, tables and images live -------------------------
KNOBS = [{}, {"MFA_WALK_C": "2"}, {"MFA_WALK_C": "2", "MFA_WALK_IMAGES_GLOBAL": "1"}, {"MFA_WALK_TABLES_GLOBAL": "1"}, {"MFA_WALK_REFILL": "4"},
         {"MFA_ACCEL": "0"}, {"MFA_WALK_LEAN": "0"}, {"MFA_WALK_LEAN": "2"}]


@pytest.mark.parametrize("k", range(24))
def test_table_engine_single_image(k, monkeypatch):
    im = corpus()[k]
    d_bytes, d_off = upload(im["strings"])
    n = len(im["strings"])
    for env in KNOBS:
        set_env(monkeypatch, dict(env, MFA_WALK="table"))
        img = capi.Image(im["blob"])
        buf = guarded(n)
        img.match_tensors(d_bytes, d_off, buf)
        what = "regex %r %s %r" % (im["regex"], im["flag"], env)
        compare(answers(buf, n, what), want_of(k), im["strings"], what)
        assert img.info()["last_kernel"] == capi.KERNEL_WALK
        img.close()


# ---- b. mixed objects, the table engine: any lane any automaton ---------------------------------------------------------------------------
def segment_sizes(n_images):
    """sizes with 0, 1, 63, 65 and 130 among them: one wave holds strings of several automata, and a segment starts inside a wave"""
    return ([63, 1, 65, 0, 130, 17, 64, 2, 129, 33, 66, 5] * 2)[:n_images]


def mixed_batch(ks, which=1):
    """the first strings of every image's batch, image by image: (strings, seg_first, wanted answers)"""
    strings, seg, want = [], [0], []
    for k, size in zip(ks, segment_sizes(len(ks))):
        strings += corpus(which)[k]["strings"][:size]
        want.append(want_of(k, which)[:size])
        seg.append(len(strings))
    if len(strings) % 64 == 0:                              # (never a multiple of 64: one string more for the last automaton)
        strings.append(corpus(which)[ks[-1]]["strings"][size])
        want.append(want_of(ks[-1], which)[size:size + 1])
        seg[-1] += 1
    return strings, seg, np.concatenate(want)


def runs_with_strings(ks, seg, which=1):
    """launches of an uncut call (walk_plan.h: plan_table_launches): one per run of consecutive segments whose automata have the same cell
    count and that holds a string -- ONE for all if an automaton of the object has more than six cells"""
    cells = [corpus(which)[k]["cells"] for k in ks]
    if max(cells) > 6:
        return 1
    runs, s0 = 0, 0
    while s0 < len(ks):
        s1 = s0
        while s1 < len(ks) and cells[s1] == cells[s0]:
            s1 += 1
        runs += seg[s1] > seg[s0]
        s0 = s1
    return runs


def by_cells(ks):
    return sorted(ks, key=lambda k: (corpus()[k]["cells"], k))


OBJECTS = {
    "A: the forward images of up to six cells": lambda: by_cells([k for k in range(12) if corpus()[k]["cells"] <= 6]),
    "A: all twelve forward images": lambda: by_cells(range(12)),
    "B: one to three cells and one of seven or more": lambda: by_cells(range(8)) + [11],
    "C: the -reverse images": lambda: list(range(18, 24)),
}


@pytest.mark.parametrize("name", list(OBJECTS))
def test_table_engine_mixed_objects(name, monkeypatch):
    walk_mixed_object(name, OBJECTS[name](), 1, name.startswith("B"), monkeypatch)


def walk_mixed_object(name, ks, which, one_launch, monkeypatch):
    strings, seg, want = mixed_batch(ks, which)
    n = len(strings)
    sizes = {0, 1, 63, 65, 130} if which == 1 or len(ks) >= 5 else {1, 63, 65}      # (an object of three automata: the first three sizes)
    assert n % 64 != 0 and sizes <= {seg[j + 1] - seg[j] for j in range(len(ks))}
    d_bytes, d_off = upload(strings)
    set_env(monkeypatch, {"MFA_WALK": "table"})
    images = [capi.Image(corpus(which)[k]["blob"]) for k in ks]
    alone = []                                              # every segment through the single-image call
    for j, img in enumerate(images):
        m = seg[j + 1] - seg[j]
        if m:
            buf = guarded(m)
            img.match_tensors(d_bytes, d_off[seg[j]:seg[j + 1] + 1], buf)
            alone.append(answers(buf, m, (name, "alone", j)))
    alone = np.concatenate(alone)
    compare(alone, want, strings, "%s, segment by segment" % name)
    mx = capi.Mixed(images)
    for cuts in ("", "0.4,0.7"):
        for cap in (None, "2"):
            set_env(monkeypatch, dict({"MFA_WALK": "table", "MFA_MIXED_CUTS": cuts}, **({"MFA_WALK_C": cap} if cap else {})))
            buf = guarded(n)
            mx.match_tensors(d_bytes, d_off, seg, d_results=buf)
            what = "%s, cuts %r, MFA_WALK_C %s" % (name, cuts, cap)
            got = answers(buf, n, what)
            compare(got, want, strings, what)
            assert np.array_equal(got, alone), what
            if not cuts:
                assert mx.last_launches()["walk_launches"] == runs_with_strings(ks, seg, which), what
                if one_launch:
                    assert mx.last_launches()["walk_launches"] == 1      # the seven-cell kernel walks all: every table with three-word edges
    mx.close()
    for img in images:
        img.close()


# ---- c. the generated kernel --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("j", range(6))
def test_specialised_engine(j, monkeypatch):
    """the six images of the corpus with the smallest generated source (the build compiled their kernels: nothing waits for a compiler here)"""
    im = regex_fuzz.specialised_six()[j]
    k = next(i for i, c in enumerate(corpus()) if c is im)
    assert im["edges"] <= 50
    d_bytes, d_off = upload(im["strings"])
    n = len(im["strings"])
    for accel in ("1", "0"):
        set_env(monkeypatch, {"MFA_WALK": "jit", "MFA_ACCEL": accel})
        img = capi.Image(im["blob"])
        buf = guarded(n)
        img.match_tensors(d_bytes, d_off, buf)
        what = "regex %r %s specialised, MFA_ACCEL=%s" % (im["regex"], im["flag"], accel)
        compare(answers(buf, n, what), want_of(k), im["strings"], what)
        assert img.info()["last_kernel"] == capi.KERNEL_SPECIALISED
        img.close()


# ---- the second corpus: cells created by a read, read marks -----------------------------------------------------------------------------------
def test_the_second_corpus_is_what_the_tests_count_on():
    c = corpus(2)
    assert len(c) == 16
    held = lambda im, *names: any(any(im["fields"][f]) for f in names)
    assert [im["cells"] for im in c[:6]] == [1, 2, 3, 4, 5, 6] and all(7 <= im["cells"] <= 9 for im in c[6:10])
    assert all(im["flag"] == "-mfa" and im["reversed"] == 0 and held(im, "c-com", "b-com") for im in c[:10])
    assert any(held(im, "c-com") for im in c[:6]) and any(held(im, "c-com") for im in c[6:10])
    assert all(im["flag"] == "-bnf" for im in c[10:13])
    assert all(im["flag"] == "-reverse" and im["reversed"] == 1 and held(im, "b-rdm") for im in c[13:])
    assert all(image.blob_info(im["blob"])["reversed"] == im["reversed"] for im in c)
    for k, im in enumerate(c):
        n = len(im["strings"])
        assert 165 <= n <= 330 and n % 64 != 0 and sum(len(s) for s in im["strings"]) < 900 * 1024
        assert 0 < want_of(k, 2).sum() < n, "%r %s: one answer only" % (im["regex"], im["flag"])


KNOBS2 = [{}, {"MFA_WALK_C": "2", "MFA_WALK_IMAGES_GLOBAL": "1"}, {"MFA_ACCEL": "0"}]


@pytest.mark.parametrize("k", range(16))
def test_table_engine_single_image_created_cells(k, monkeypatch):
    im = corpus(2)[k]
    d_bytes, d_off = upload(im["strings"])
    n = len(im["strings"])
    for env in KNOBS2:
        set_env(monkeypatch, dict(env, MFA_WALK="table"))
        img = capi.Image(im["blob"])
        buf = guarded(n)
        img.match_tensors(d_bytes, d_off, buf)
        what = "regex %r %s %r" % (im["regex"], im["flag"], env)
        compare(answers(buf, n, what), want_of(k, 2), im["strings"], what)
        assert img.info()["last_kernel"] == capi.KERNEL_WALK
        img.close()


OBJECTS2 = {
    "D: one to six cells, created open": lambda: list(range(6)),
    "E: the same six and one of seven or more cells": lambda: list(range(6)) + [6],
    "F: the -reverse images, read marks": lambda: [13, 14, 15],
}


@pytest.mark.parametrize("name", list(OBJECTS2))
def test_table_engine_mixed_objects_created_cells(name, monkeypatch):
    """E takes ONE launch: the six automata of one to six cells are walked by the nine-cell kernel, every table with three-word edges, lanes
    of different automata in one wave"""
    walk_mixed_object(name, OBJECTS2[name](), 2, name.startswith("E"), monkeypatch)


def test_the_specialised_eight_are_what_the_tests_count_on():
    eight = [im for _, im in regex_fuzz.specialised_eight()]
    assert len(eight) == 8 and all(im["edges"] <= 50 for im in eight)
    for name, has in regex_fuzz.SPEC2_KINDS.items():
        assert any(has(im) for im in eight), name


@pytest.mark.parametrize("j", range(8))
def test_specialised_engine_created_cells(j, monkeypatch):
    """eight images of the second corpus through the generated kernel (the build compiled their kernels): a cell created open in a byte-class
    list and in a waiting list (phase C), a reversed scan, four cells or more among them"""
    im = regex_fuzz.specialised_eight()[j][1]
    k = next(i for i, c in enumerate(corpus(2)) if c is im)
    d_bytes, d_off = upload(im["strings"])
    n = len(im["strings"])
    for accel in ("1", "0"):
        set_env(monkeypatch, {"MFA_WALK": "jit", "MFA_ACCEL": accel})
        img = capi.Image(im["blob"])
        buf = guarded(n)
        img.match_tensors(d_bytes, d_off, buf)
        what = "regex %r %s specialised, MFA_ACCEL=%s" % (im["regex"], im["flag"], accel)
        compare(answers(buf, n, what), want_of(k, 2), im["strings"], what)
        assert img.info()["last_kernel"] == capi.KERNEL_SPECIALISED
        img.close()
