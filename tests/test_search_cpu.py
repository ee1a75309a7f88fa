"""Search inside lines, the part that can be wrong without a GPU: the two tables csrc/search_tables.cpp derives from an image's tabulated
table and the walk of one lane over them (csrc/search_core.h), compiled for the host (tests/emul/search/search_emul.cpp) -- against the
definition (the oracle's whole-string match on every substring), against a brute force on the image's own table for longer lines, on
the corners, under the host sanitizers; the plan of a call; and the refusals of the C-ABI, which need no device.  The kernels around
the walk are checked by tests/test_search_gpu.py against the same harness."""
import ctypes
import os
import re

import numpy as np
import pytest

import oracle_lib
import search_lib
import testlib
from mfa_amd import capi, image

SEED = 20261021


@pytest.fixture(scope="module")
def exe():
    return search_lib.search_exe()


@pytest.fixture(scope="module")
def imgs(tmp_path_factory):
    return search_lib.images(tmp_path_factory.mktemp("search_images"))


def test_images_are_the_ones_asked_for(imgs):
    assert len(testlib.NFA_NAMES) == 26 and "nfa_star3_plain" not in testlib.NFA_NAMES
    assert len(imgs) == 2 * 26 + 5
    assert search_lib.info_reversed(imgs["table_66_rev"][0]) == 1 and search_lib.info_reversed(imgs["table_66_fwd"][0]) == 0


def test_definition_against_the_oracle(exe, imgs, tmp_path):
    """300 short strings per image: the harness's results, spans and span results against the leftmost-longest pair among all substrings
    the oracle accepts.  Every image has lines with a match and lines without, unless its language holds the empty string."""
    for k, (name, (blob, alpha)) in enumerate(sorted(imgs.items())):
        rng = np.random.default_rng(SEED + k)
        strings = search_lib.short_strings(name, alpha, rng)
        want = search_lib.oracle_spans(blob, strings)
        res, spans, sres = search_lib.emul_run(exe, blob, strings, tmp_path)
        w_res, w_spans, w_sres = search_lib.expected_outputs(strings, want)
        bad = np.nonzero(res != w_res)[0]
        assert bad.size == 0, "%s: %d results differ, first line %d %r" % (name, bad.size, bad[0], strings[bad[0]])
        bad = np.nonzero(spans != w_spans)[0]
        assert bad.size == 0, "%s: span word %d of line %r: want %d got %d" % (name, bad[0], strings[bad[0] // 2], w_spans[bad[0]], spans[bad[0]])
        assert np.array_equal(sres, w_sres), name
        has_empty = bool(oracle_lib.OracleImage(blob).match([b""])[0])
        found = int(w_res.sum())
        if has_empty:
            assert found == len(strings) and all(i == 0 for _, i, _ in want), name
        else:
            assert 0 < found < len(strings), "%s: %d of %d lines have a match" % (name, found, len(strings))


def _long_batches(imgs):
    for k, (name, (blob, alpha)) in enumerate(sorted(imgs.items())):
        yield name, blob, search_lib.long_strings(name, alpha, np.random.default_rng(SEED + 1000 + k))


def test_longer_lines_against_brute_force(exe, imgs, tmp_path):
    """lines of 0 to 4097 bytes that start at every offset mod 16, in a buffer of exactly the readable room: the walks against a brute
    force inside the harness on the image's own table (a difference is the harness's exit code 5)"""
    for name, blob, strings in _long_batches(imgs):
        assert len({o % 16 for o in testlib.out_offsets(strings)}) == 16 and max(len(s) for s in strings) == 4097
        res, spans, sres = search_lib.emul_run(exe, blob, strings, tmp_path, check=True)
        assert set(res.tolist()) <= {0, 1} and np.all(spans[1:] >= spans[:-1]), name
        assert np.array_equal(sres[0::2], res) and not sres[1::2].any(), name


def test_under_sanitizers(imgs, tmp_path):
    """the same batches with the harness built with -fsanitize=address,undefined (a plain executable, nothing preloaded): no walk reads
    outside the aligned 16-byte blocks its line touches"""
    exe = search_lib.search_exe("-fsanitize=address,undefined -fno-sanitize-recover=all")
    for name, blob, strings in _long_batches(imgs):
        search_lib.emul_run(exe, blob, strings, tmp_path, check=True)


def test_corners(exe, imgs, tmp_path):
    abb = testlib.fixture_blob("nfa_abb_thompson", 0)                    # (a|b)*abb
    for blob in (abb, testlib.fixture_blob("nfa_abb_thompson", 1)):
        rev = search_lib.info_reversed(blob)
        word = b"bba" if rev else b"abb"
        # n == 0
        res, spans, sres = search_lib.emul_run(exe, blob, [], tmp_path)
        assert res.size == 0 and sres.size == 0 and list(spans) == [0]
        # empty lines between others; a match that is the whole line; a match of the last bytes only; none
        strings = [b"", word, b"", b"zzz" + word, b"zz", b"", (word + b"a" if rev else b"a" + word) + b"z"]
        res, spans, sres = search_lib.emul_run(exe, blob, strings, tmp_path, check=True)
        assert list(res) == [0, 1, 0, 1, 0, 0, 1]
        off = testlib.out_offsets(strings) + [sum(len(s) for s in strings)]
        assert (spans[2], spans[3]) == (off[1], off[2])                  # the whole line
        assert (spans[6], spans[7]) == (off[3] + 3, off[4])              # its last three bytes
        assert (spans[12], spans[13]) == (off[6], off[6] + 4)            # leftmost begin, longest end short of the z
        for k in (0, 2, 4, 5):
            assert spans[2 * k] == spans[2 * k + 1] == off[k]
        assert spans[-1] == off[-1] and list(sres) == [0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0]
    # a match of the last byte only
    for rev in (0, 1):
        res, spans, _ = search_lib.emul_run(exe, testlib.front_end_blob("a", tmp_path, rev), [b"zzzzzzzzzzzzzzzzzzza", b"az"], tmp_path, check=True)
        assert list(res) == [1, 1] and list(spans) == [19, 20, 20, 21, 22]
    # a language with the empty string: every line is found at its begin, with the longest match that begins there
    strings = [b"zzz", b"", b"abab", b"z" * 40, b"ababaz", b"zab"]
    for regex, ends in (("(ab)*", [0, 0, 4, 0, 4, 0]), ("(a|b)*", [0, 0, 4, 0, 5, 0]), ("a*", [0, 0, 1, 0, 1, 0])):
        for rev in (0, 1):
            blob = testlib.front_end_blob(regex, tmp_path, rev)
            assert oracle_lib.OracleImage(blob).match([b""])[0] == 1
            res, spans, _ = search_lib.emul_run(exe, blob, strings, tmp_path, check=True)
            off = testlib.out_offsets(strings)
            if rev and regex == "(ab)*":
                ends = [0] * 6                                          # the mirrored language (ba)*: nothing but the empty match begins a line here
            assert list(res) == [1] * 6 and list(spans[0:12:2]) == off and list(spans[1:12:2]) == [o + e for o, e in zip(off, ends)], (regex, rev)
            want = search_lib.expected_outputs(strings, search_lib.oracle_spans(blob, strings))
            assert np.array_equal(res, want[0]) and np.array_equal(spans, want[1]), (regex, rev)
            info = search_lib.emul_info(exe, blob, tmp_path)
            assert info[0][1] == 1 and info[0][2] == info[1][2] == 1, (regex, rev)      # an injecting table whose start set accepts: every set does


def test_numbering_of_both_tables(exe, imgs, tmp_path):
    """0 the dead set, 1 the start set, accepting sets highest: accept_from splits the numbers, a start set that accepts stays at 1 (below
    accept_from unless every set accepts) and is then entered by no byte; a plain table's dead set is absorbing.  Sizes as counted."""
    sizes = {}
    for name, (blob, _) in sorted(imgs.items()):
        info = search_lib.emul_info(exe, blob, tmp_path)
        assert info is not None, name
        for p, (states, accept_from, start_accepts, enters_start, row0_dead) in enumerate(info):
            assert 2 <= states <= 127 and 1 <= accept_from <= states, (name, p)
            if accept_from == 1:
                assert start_accepts, (name, p)
            elif start_accepts:
                assert not enters_start, (name, p)
        assert info[1][4] == 1, name                                     # pass 2 stops at the dead set
        has_empty = bool(oracle_lib.OracleImage(blob).match([b""])[0])
        assert info[0][2] == info[1][2] == int(has_empty), name
        if has_empty:
            assert info[0][1] == 1, name                                 # an injecting table whose start set accepts: every set does
        sizes[name] = (info[0][0], info[1][0])
    assert sizes["table_66_fwd"] == (8, 66) and sizes["table_66_rev"] == (66, 8)
    assert sizes["table_127_fwd"] == (20, 127) and sizes["table_127_rev"] == (127, 48)
    assert sizes["ab5a_fwd"] == (65, 13)
    fixtures = [v for k, v in sizes.items() if k.startswith("nfa_")]
    assert min(a for a, _ in fixtures) >= 3 and max(a for a, _ in fixtures) <= 25 and max(b for _, b in fixtures) <= 14


def test_plan(exe):
    """tiled exactly when table + tile <= 64 KiB; grids within what the CUs keep resident"""
    seen = set()
    for s1 in (0, 2, 3, 25, 55, 56, 66, 127):
        for s2 in (0, 2, 66, 127):
            for n in (1, 255, 256, 257, 100000, 1 << 22):
                for cus in (1, 256):
                    p = search_lib.emul_plan(exe, s1, s2, n, cus)
                    table = s1 * 258 * 2
                    assert p["tile"] == 4 * 64 * 144
                    assert p["form"] == ("tiled" if table + p["tile"] <= 65536 else "untiled")
                    assert p["lds1"] == (table + p["tile"] if p["form"] == "tiled" else table) <= 65536 and p["lds2"] == s2 * 258 * 2
                    want = lambda lds: max(1, min(8, 160 * 1024 // max(lds, 1)))
                    assert p["per_cu1"] == want(p["lds1"]) and p["per_cu2"] == want(p["lds2"])
                    for grid, per_cu in ((p["grid1"], p["per_cu1"]), (p["grid2"], p["per_cu2"])):
                        assert 1 <= grid <= cus * per_cu and grid == min((n + 255) // 256, cus * per_cu)
                    seen.add(p["form"])
    assert seen == {"tiled", "untiled"}
    assert search_lib.emul_plan(exe, 55, 2, 1, 1)["form"] == "tiled" and search_lib.emul_plan(exe, 56, 2, 1, 1)["form"] == "untiled"


def test_no_scratch():
    """every kernel of search.o: 0 bytes of scratch (search.log is what the build leaves)"""
    log = os.path.join(testlib.CSRC, "search.log")
    if os.path.exists(log):
        with open(log) as f:
            text = f.read()
        names = re.findall(r"Function Name: (\S+)", text)
        sizes = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)
        assert len(names) == 3 and len(sizes) == 3 and all(s == "0" for s in sizes), list(zip(names, sizes))


# ---- the C-ABI without a device -----------------------------------------------------------------------------------------------------------
def _fake(n=4096):
    """host memory standing in for device memory, filled with 7: the calls below return before they would touch it"""
    buf = (ctypes.c_uint8 * (n + 64))(*([7] * (n + 64)))
    return buf, (ctypes.addressof(buf) + 63) // 64 * 64


def _search(img, p, n=8, bytes_=0, offsets=256, results=512, spans=1024, sres=2048):
    at = lambda x: None if x is None else p + x
    return capi.lib().mfa_search_batch(img._h if img is not None else None, at(bytes_), at(offsets), n, at(results), at(spans), at(sres), 0, None)


def test_exports():
    for name in ("mfa_search_batch", "mfa_search_batch_host", "mfa_image_search_info"):
        assert hasattr(capi.lib(), name) and name in capi.EXPORTS
    with open(os.path.join(oracle_lib.ROOT, "include", "mfa_hip.h")) as f:
        hdr = f.read()
    assert re.search(r"#define\s+MFA_KERNEL_SEARCH\s+\(MFA_KERNEL_NODESET \+ 1u\)", hdr) and capi.KERNEL_SEARCH == capi.KERNEL_NODESET + 1 == 5


def _refused(tmp_path, monkeypatch):
    out = {"ex1_plain": capi.Image(image.blob_from_dump(oracle_lib.load_dump("ex1_plain")))}
    monkeypatch.setenv("MFA_NFA_SETWALK", "1")
    out["setwalk"] = capi.Image(testlib.fixture_blob("nfa_abb_thompson"))
    monkeypatch.delenv("MFA_NFA_SETWALK")
    out["t514"] = capi.Image(testlib.table_blob("t514", tmp_path))
    out["ab8a"] = capi.Image(testlib.front_end_blob("(a|b)" * 8 + "a", tmp_path))
    return out


def test_refusals_without_a_device(tmp_path, monkeypatch):
    """a memory automaton, a set-walk image, an image of more than 127 state sets, one whose pass 1 table passes 127: MFA_ERR_UNSUPPORTED
    before the device is touched, every output as it was; so are the argument errors"""
    keep, p = _fake()
    before = bytes(keep)
    refused = _refused(tmp_path, monkeypatch)
    assert refused["setwalk"].info()["dfa_states"] == 0 and refused["t514"].info()["dfa_states"] == 514 and refused["ab8a"].info()["dfa_states"] <= 127
    for name, img in refused.items():
        assert _search(img, p) == capi.ERR_UNSUPPORTED, name
        assert _search(img, p, n=0) == capi.ERR_UNSUPPORTED, name
        assert _search(img, p, spans=None, sres=None) == capi.ERR_UNSUPPORTED, name
        with pytest.raises(capi.MfaError) as e:
            img.search_info()
        assert e.value.code == capi.ERR_UNSUPPORTED, name
        with pytest.raises(capi.MfaError) as e:
            img.search_host(np.zeros(16, dtype=np.uint8), np.array([0, 3, 5], dtype=np.uint64))
        assert e.value.code == capi.ERR_UNSUPPORTED, name
    good = capi.Image(testlib.fixture_blob("nfa_abb_thompson"))
    bad = capi.ERR_INVALID_ARG
    assert _search(None, p) == bad and _search(good, p, offsets=None) == bad and _search(good, p, results=None) == bad
    assert _search(good, p, spans=None) == bad                           # span results without spans
    for k in (1, 2, 4, 7):
        assert _search(good, p, spans=1024 + k) == bad
    assert bytes(keep) == before
    # what is well-formed passes the checks: without a device the next answer is "no device"
    if capi.device_count() <= 0:
        assert _search(good, p) == capi.ERR_NO_DEVICE and _search(good, p, spans=None, sres=None) == capi.ERR_NO_DEVICE
        assert _search(good, p, n=0, spans=None, sres=None) == capi.OK
        assert bytes(keep) == before
    assert all(3 <= s <= 25 for s in good.search_info())
    for img in list(refused.values()) + [good]:
        img.close()
    del keep
