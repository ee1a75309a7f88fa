"""Batch to text, the part that can be wrong without a GPU (csrc/select_core.h: the kept rule, the workspace, the geometry of an output
tile, the searches in the output offsets, a chunk's way from aligned source blocks through the staging area to the destination),
compiled for the host (tests/emul/select_emul.cpp) and run block by block and tile by tile in the kernels' order, against the rule
restated in Python (tests/select_lib.py: expected).  The ABI's argument checks, which need no device, are here too.  The kernels around
the core are checked by tests/test_select_gpu.py on the same cases."""
import ctypes
import os
import re

import numpy as np
import pytest

from mfa_amd import capi
from select_lib import (ALL_FLAGS, INVERT, NEWLINE, all_cases, case, check_against_python, emul_results, expected, geometry)
from testlib import CSRC, emul_exe

B, T, SCAN_ROUND = geometry()


@pytest.fixture(scope="module")
def cases():
    return all_cases()


def test_geometry_is_what_the_header_says():
    assert B == 1024 and T == 16384 and SCAN_ROUND == 4096 * 1024


def test_rule_edges():
    """the examples of the rule, in Python's terms: what every other test compares with"""
    c = case("x", [b"ab", b"", b"cde", b"f"], [1, 1, 0, 2])
    info, off, ind, data = expected(c.data, c.off, c.res, 0, 4, 100)
    assert (info["n_selected"], info["n_bytes"], info["n_unanswered"], info["overflow"]) == (2, 2, 1, 0)
    assert list(off) == [0, 2, 2] and list(ind) == [0, 1] and data == b"ab"
    info, off, ind, data = expected(c.data, c.off, c.res, NEWLINE, 4, 100)
    assert info["n_bytes"] == 4 and list(off) == [0, 3, 4] and data == b"ab\n\n"
    info, off, ind, data = expected(c.data, c.off, c.res, INVERT | NEWLINE, 4, 100)
    assert info["n_selected"] == 1 and info["n_unanswered"] == 1 and list(ind) == [2] and data == b"cde\n"
    # clipped: the counts stay true, offsets up to v, bytes up to the capacity
    info, off, ind, data = expected(c.data, c.off, c.res, NEWLINE, 1, 2)
    assert (info["n_selected"], info["n_bytes"], info["overflow"]) == (2, 4, 1) and list(off) == [0, 3] and list(ind) == [0] and data == b"ab"


def test_cases_cover_what_they_are_for(cases):
    names = [c.name for c in cases]
    assert len([n for n in names if n.startswith("random_")]) >= 200 and len([n for n in names if n.startswith("align_")]) == 256
    assert {(int(c.src_shift + c.off[0]) % 16, c.dst_shift) for c in cases if c.name.startswith("align_")} == {(a, d) for a in range(16) for d in range(16)}
    assert any(len(c.res) > SCAN_ROUND for c in cases) and {B - 1, B, B + 1} <= {len(c.res) for c in cases}
    assert any(c.src_shift for c in cases) and any(not c.with_indices for c in cases)
    infos = [expected(c.data, c.off, c.res, c.flags, c.max_selected, c.capacity)[0] for c in cases if "_clip_" in c.name]
    assert sum(i["overflow"] for i in infos) > len(infos) // 2 and any(not i["overflow"] for i in infos)


def test_harness_against_python(cases, tmp_path):
    check_against_python(emul_results(emul_exe("select"), tmp_path, cases), cases, "harness")


def test_under_sanitizers(cases, tmp_path):
    """the same cases once more with the harness built with -fsanitize=address,undefined (a plain executable, nothing preloaded): the
    strings lie in exactly the aligned 16-byte blocks they touch and every output in exactly its capacity"""
    exe = emul_exe("select", "-fsanitize=address,undefined -fno-sanitize-recover=all")
    check_against_python(emul_results(exe, tmp_path, cases), cases, "sanitized")


def test_no_scratch():
    """every kernel of select.o: 0 bytes of scratch (select.log is what the build leaves)"""
    log = os.path.join(CSRC, "select.log")
    if os.path.exists(log):
        with open(log) as f:
            text = f.read()
        names = re.findall(r"Function Name: (\S+)", text)
        sizes = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)
        assert len(names) == 4 and len(sizes) == 4 and all(s == "0" for s in sizes), list(zip(names, sizes))


# ---- the ABI's argument checks: answered before a device is touched -----------------------------------------------------------------------
def _fake(n=256):
    """host memory standing in for device memory: the calls below return before they would touch it"""
    buf = ctypes.create_string_buffer(n + 64)
    return buf, (ctypes.addressof(buf) + 63) // 64 * 64


def test_exports_and_sizes():
    L = capi.lib()
    for name in ("mfa_select_workspace_bytes", "mfa_select_count", "mfa_select_write"):
        assert hasattr(L, name) and name in capi.EXPORTS
    assert ctypes.sizeof(capi.SelectInfo) == 32
    assert (capi.SELECT_INVERT, capi.SELECT_NEWLINE) == (INVERT, NEWLINE)
    sizes = [capi.select_workspace_bytes(n) for n in (0, 1, B, B + 1, 1 << 30)]
    assert sizes[0] >= 16 and sizes[1] == sizes[2] and sizes[3] > sizes[2] and all(s % 16 == 0 for s in sizes)
    assert sizes[4] < 3 * (1 << 30)                       # a few bytes per string
    assert L.mfa_select_workspace_bytes(10, None) == capi.ERR_INVALID_ARG
    out = ctypes.c_size_t()
    assert L.mfa_select_workspace_bytes(1 << 40, ctypes.byref(out)) == capi.ERR_INVALID_ARG
    assert L.mfa_select_workspace_bytes((1 << 40) - 1, ctypes.byref(out)) == capi.OK


def test_argument_checks():
    L = capi.lib()
    keep, p = _fake(2048)
    results, offsets, work, info, src, out_bytes, out_off, out_ind = p, p + 256, p + 512, p + 1024, p + 1088, p + 1280, p + 1536, p + 1792
    count = lambda results=results, offsets=offsets, n=8, flags=0, work=work, info=info: L.mfa_select_count(results, offsets, n, flags, work, info, 0, None)
    write = lambda src=src, offsets=offsets, results=results, n=8, flags=0, work=work, info=info, out=out_bytes, cap=64, off=out_off, ind=out_ind, ms=4: \
        L.mfa_select_write(src, offsets, results, n, flags, work, info, out, cap, off, ind, ms, 0, None)
    bad = capi.ERR_INVALID_ARG
    # NULL pointers
    assert count(results=None) == bad and count(offsets=None) == bad and count(work=None) == bad and count(info=None) == bad
    assert write(src=None) == bad and write(offsets=None) == bad and write(results=None) == bad and write(work=None) == bad
    assert write(info=None) == bad and write(out=None) == bad and write(off=None) == bad
    # unknown flag bits
    for flags in (4, 8, 0x80000000, 0xffffffff):
        assert count(flags=flags) == bad and write(flags=flags) == bad
    # alignment: the workspace on 16 bytes; the info record, the offsets and the two 8-byte outputs on 8
    assert count(work=work + 8) == bad and write(work=work + 8) == bad
    for k in (1, 4, 7):
        assert count(info=info + k) == bad and count(offsets=offsets + k) == bad
        assert write(info=info + k) == bad and write(offsets=offsets + k) == bad and write(off=out_off + k) == bad and write(ind=out_ind + k) == bad
    # 2^40 strings and more
    assert count(n=1 << 40) == bad and write(n=1 << 40) == bad and count(n=(1 << 64) - 1) == bad
    # what is well-formed passes the checks: here, without a device, the next answer is "no device"
    if capi.device_count() <= 0:
        ok = (capi.ERR_NO_DEVICE,)
        assert count() in ok and count(flags=3) in ok and count(n=0) in ok
        assert write() in ok and write(out=None, cap=0) in ok and write(ind=None) in ok and write(src=src + 3, out=out_bytes + 5) in ok
    # a device index out of range is "no device" with or without one
    assert L.mfa_select_count(results, offsets, 8, 0, work, info, 1 << 20, None) == capi.ERR_NO_DEVICE
    assert L.mfa_select_write(src, offsets, results, 8, 0, work, info, out_bytes, 64, out_off, out_ind, 4, -1, None) == capi.ERR_NO_DEVICE
    del keep
