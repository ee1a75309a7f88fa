"""Text to batch, the part that can be wrong without a GPU (csrc/text_split_core.h: the separator masks of a 16-byte block, the marks, a
tile's totals, the write position of a kept byte and of an offset, the stop-token comparison, the plan of the aligned stores), compiled
for the host (tests/emul/text_split_emul.cpp) and run block by block in the kernels' order.  The rule is pinned on two sides: against
Python (bytes.split(); split(b"\\n") minus a trailing empty element) and against libstdc++ itself (tests/emul/iostream_split.cpp:
`cin >> s` and getline over the same texts).  The ABI's argument checks, which need no device, are here too.  The kernels around the
core are checked by tests/test_text_split_gpu.py."""
import ctypes
import struct
import subprocess

import numpy as np
import pytest

from mfa_amd import capi
from testlib import EMUL_DIR, emul_exe
from textsplit_lib import (LINES, STOP, TOKENS, both_modes, edge_texts, emul_results, expected, py_split, random_texts, tile_bytes)

T = tile_bytes()


@pytest.fixture(scope="module")
def emul():
    return emul_exe("text_split")


@pytest.fixture(scope="module")
def iostream_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("iostream_split") / "iostream_split")
    p = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, "iostream_split.cpp"], cwd=EMUL_DIR, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    return exe


def check_cases(results, cases, what):
    assert len(results) == len(cases)
    for k, ((info, off, data, _), (text, mode, stop, max_strings, capacity)) in enumerate(zip(results, cases)):
        w_info, w_off, w_data = expected(text, mode, stop, len(text) + 1 if max_strings is None else max_strings,
                                         len(text) if capacity is None else capacity)
        tag = "%s case %d (mode %d, %d bytes)" % (what, k, mode, len(text))
        assert info == w_info, tag
        assert np.array_equal(off, w_off), tag
        assert data == w_data, tag


def test_tile_is_what_the_header_says():
    assert T == 16384 and T % 1024 == 0


def test_rule_edges():
    """the examples of the rule, in Python's terms: what every other test compares with"""
    assert py_split(b"", LINES)[0] == [] and py_split(b"\n", LINES)[0] == [b""]
    assert py_split(b"a\nb", LINES)[0] == py_split(b"a\nb\n", LINES)[0] == [b"a", b"b"]
    assert py_split(b"a\r\n\x00\n\n", LINES)[0] == [b"a\r", b"\x00", b""]
    assert py_split(b" a\x0bb\x0cc\rd\te\nf ", TOKENS)[0] == [b"a", b"b", b"c", b"d", b"e", b"f"]
    assert py_split(b"a exits xexit exit b", TOKENS, STOP) == ([b"a", b"exits", b"xexit"], True)
    assert py_split(b"a exit", TOKENS, STOP) == ([b"a"], True) and py_split(b"a exi", TOKENS, STOP) == ([b"a", b"exi"], False)


def test_edges_and_tile_borders(emul, tmp_path):
    texts = edge_texts(T)
    cases = both_modes(list(texts.values())) + [(t, TOKENS, None, None, None) for t in texts.values()]
    check_cases(emul_results(emul, tmp_path, cases), cases, "edges")
    # the stop token does what its cases are named for
    names = list(texts)
    stopped = {n: r[0]["stopped"] for n, r in zip(names, emul_results(emul, tmp_path, [(texts[n], TOKENS, STOP, None, None) for n in names]))}
    for n in names:
        want = n.startswith("stop_") and n not in ("stop_not", "stop_prefix_at_end", "stop_long_tail")
        assert stopped[n] == int(want), n


def test_random_texts(emul, tmp_path):
    """300 seeded texts of 0 to 5 tiles, both modes"""
    cases = both_modes(random_texts(T))
    results = emul_results(emul, tmp_path, cases)
    check_cases(results, cases, "random")
    assert sum(r[0]["stopped"] for r in results) > 30 and sum(1 for r in results[300:] if not r[0]["stopped"]) > 30


def test_other_stop_tokens(emul, tmp_path):
    """1 byte, 8 and 9 (the two words of the packed token), 15 bytes; bytes of 0x80 and more"""
    cases = []
    for stop in (b"q", b"12345678", b"123456789", b"123456789abcdef", b"\xff\x80z"):
        body = b"a " + stop + b"x " + b"y" + stop + b" " + stop[:-1] + b" "
        cases += [(body + stop + b" tail", TOKENS, stop, None, None), (body + stop, TOKENS, stop, None, None), (body, TOKENS, stop, None, None),
                  ((b"ab " * 6000)[:T - len(stop)] + b" " + stop + b"\nq", TOKENS, stop, None, None)]      # (the token's last byte opens the next tile)
    results = emul_results(emul, tmp_path, cases)
    check_cases(results, cases, "stop tokens")
    assert [r[0]["stopped"] for r in results] == [1, 1, 0, 1] * 5


def test_clipped_writes(emul, tmp_path):
    """capacities that are too small, one and both: the counts stay true, overflow is set, what fits is written (the harness holds the
    buffers in exactly their capacities, which the sanitizer run below watches)"""
    texts = random_texts(T, count=12, seed=7) + [edge_texts(T)["long_string"], b"a b c", b""]
    cases = []
    for t in texts:
        for mode, stop in ((LINES, None), (TOKENS, STOP)):
            strings, _ = py_split(t, mode, stop)
            n, nb = len(strings), sum(len(s) for s in strings)
            cases += [(t, mode, stop, n // 2, None), (t, mode, stop, None, nb // 2), (t, mode, stop, n // 3, nb // 3), (t, mode, stop, 0, 0),
                      (t, mode, stop, n, nb), (t, mode, stop, max(n, 1) - 1, max(nb - 1, 0))]
    results = emul_results(emul, tmp_path, cases)
    check_cases(results, cases, "clipped")
    assert sum(r[0]["overflow"] for r in results) > len(cases) // 2


def test_against_libstdcxx(emul, iostream_exe, tmp_path):
    """`cin >> s` and getline over the edge texts and 60 of the random ones give the strings the harness gives"""
    texts = list(edge_texts(T).values()) + random_texts(T)[:60]
    cases = both_modes(texts)
    results = emul_results(emul, tmp_path, cases)
    for (info, off, data, _), (text, mode, stop, _, _) in zip(results, cases):
        cmd = [iostream_exe, "lines"] if mode == LINES else [iostream_exe, "tokens", stop.decode()]
        raw = subprocess.run(cmd, input=text, capture_output=True, check=True).stdout
        n = struct.unpack_from("<Q", raw, 0)[0]
        at, strings = 8, []
        for _ in range(n):
            ln = struct.unpack_from("<Q", raw, at)[0]
            strings.append(raw[at + 8:at + 8 + ln])
            at += 8 + ln
        assert info["n_strings"] == n and data == b"".join(strings)
        assert [int(x) for x in off] == [0] + [int(x) for x in np.cumsum([len(s) for s in strings])]


def test_under_sanitizers(tmp_path):
    """the harness once more as a stand-alone program built with -fsanitize=address,undefined (a plain executable, nothing preloaded): the
    edge texts, 40 random ones and the clipped cases, with the text, d_bytes and d_offsets in exactly the room they are promised"""
    exe = emul_exe("text_split", "-fsanitize=address,undefined -fno-sanitize-recover=all")
    texts = list(edge_texts(T).values()) + random_texts(T)[:40]
    cases = both_modes(texts)
    for t in texts[:50]:
        for mode, stop in ((LINES, None), (TOKENS, STOP)):
            strings, _ = py_split(t, mode, stop)
            n, nb = len(strings), sum(len(s) for s in strings)
            cases += [(t, mode, stop, n // 2, nb // 2), (t, mode, stop, 0, 0), (t, mode, stop, n, nb)]
    check_cases(emul_results(exe, tmp_path, cases), cases, "sanitized")


# ---- the ABI's argument checks: answered before a device is touched -----------------------------------------------------------------------
def _fake(n=256):
    """host memory standing in for device memory: the calls below return before they would touch it"""
    buf = ctypes.create_string_buffer(n + 64)
    return buf, (ctypes.addressof(buf) + 63) // 64 * 64


def test_exports_and_sizes():
    L = capi.lib()
    for name in ("mfa_split_tile_bytes", "mfa_split_workspace_bytes", "mfa_split_text_count", "mfa_split_text_write"):
        assert hasattr(L, name) and name in capi.EXPORTS
    assert capi.split_tile_bytes() == T
    assert ctypes.sizeof(capi.SplitInfo) == 32
    assert capi.split_workspace_bytes(0) >= 32 and capi.split_workspace_bytes(T) == 32 and capi.split_workspace_bytes(T + 1) == 64
    assert capi.split_workspace_bytes(1 << 30) == 32 * ((1 << 30) // T)
    assert L.mfa_split_workspace_bytes(10, None) == capi.ERR_INVALID_ARG
    out = ctypes.c_size_t()
    assert L.mfa_split_workspace_bytes(1 << 46, ctypes.byref(out)) == capi.ERR_INVALID_ARG


def test_argument_checks():
    L = capi.lib()
    keep, p = _fake(1024)
    text, work, info, out_bytes, offsets = p, p + 256, p + 512, p + 640, p + 768
    count = lambda text=text, n=100, mode=TOKENS, stop=None, work=work, info=info: L.mfa_split_text_count(text, n, mode, stop, work, info, 0, None)
    write = lambda text=text, n=100, mode=TOKENS, work=work, info=info, out=out_bytes, cap=64, off=offsets, ms=4: L.mfa_split_text_write(
        text, n, mode, work, info, out, cap, off, ms, 0, None)
    bad = capi.ERR_INVALID_ARG
    # NULL pointers
    assert count(text=None) == bad and count(work=None) == bad and count(info=None) == bad
    assert write(text=None) == bad and write(work=None) == bad and write(info=None) == bad and write(out=None) == bad and write(off=None) == bad
    # an unknown mode
    assert count(mode=2) == bad and write(mode=2) == bad and count(mode=0xffffffff) == bad
    # the stop token: in lines mode, empty, 16 bytes, a separator inside
    assert count(mode=LINES, stop=b"exit") == bad
    assert count(stop=b"") == bad and count(stop=b"0123456789abcdef") == bad
    for sep in b" \t\n\r\x0b\x0c":
        assert count(stop=b"ex" + bytes([sep]) + b"it") == bad
    # a text that is not 16-byte aligned
    for k in (1, 4, 8, 15):
        assert count(text=text + k) == bad and write(text=text + k) == bad
    assert count(work=work + 8) == bad and count(info=info + 4) == bad and write(off=offsets + 4) == bad
    # what is well-formed passes the checks: here, without a device, the next answer is "no device"
    ok = (capi.OK, capi.ERR_NO_DEVICE) if capi.device_count() > 0 else (capi.ERR_NO_DEVICE,)
    if capi.device_count() <= 0:
        assert count() in ok and count(stop=b"exit") in ok and count(stop=b"0123456789abcde") in ok and count(mode=LINES) in ok
        assert write() in ok and write(out=None, cap=0) in ok and count(text=None, n=0) in ok
    # a device index out of range is "no device" with or without one
    assert L.mfa_split_text_count(text, 100, TOKENS, None, work, info, 1 << 20, None) == capi.ERR_NO_DEVICE
    assert L.mfa_split_text_write(text, 100, TOKENS, work, info, out_bytes, 64, offsets, 4, -1, None) == capi.ERR_NO_DEVICE
    del keep
