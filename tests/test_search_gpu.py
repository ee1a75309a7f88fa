"""Search inside lines on the GPU (csrc/search.hip behind mfa_search_batch): results, spans and span results byte for byte against the host
harness tests/emul/search/search_emul.cpp -- which tests/test_search_cpu.py holds to the oracle -- with guard bytes around all three outputs;
both kernel forms of pass 1; results only; a line beyond the limit; the spans as a batch for the selection; the round trip from a text
to the lines Python keeps; a stream capture; the refusals on real buffers; the command line against Python."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import oracle_lib
import search_lib
import testlib
from mfa_amd import capi, image

pytestmark = pytest.mark.gpu
SEED = 20261021
FRONT = 64                                                  # guard bytes (8 guard words) in front of and behind every output


@pytest.fixture(scope="module")
def exe():
    return search_lib.search_exe()


@pytest.fixture(scope="module")
def imgs(tmp_path_factory):
    return search_lib.images(tmp_path_factory.mktemp("search_images"))


class Room:
    """the three outputs of a batch of n lines, every byte 7, with guards in front of and behind each"""

    def __init__(self, n, spans=True, span_results=True):
        self.n = n
        self.res = torch.full((FRONT + max(n, 1) + FRONT,), 7, dtype=torch.uint8, device="cuda")
        self.spans = torch.full((8 + 2 * n + 1 + 8,), 0x0707070707070707, dtype=torch.int64, device="cuda") if spans else None
        self.sres = torch.full((FRONT + max(2 * n, 1) + FRONT,), 7, dtype=torch.uint8, device="cuda") if span_results else None

    def args(self):
        n = self.n
        return (self.res[FRONT:FRONT + max(n, 1)], self.spans[8:8 + 2 * n + 1] if self.spans is not None else None,
                self.sres[FRONT:FRONT + max(2 * n, 1)] if self.sres is not None else None)

    def read(self):
        """(results, spans, span results) after the guards have been looked at"""
        n = self.n
        res = self.res.cpu().numpy()
        assert (res[:FRONT] == 7).all() and (res[FRONT + n:] == 7).all(), "a byte outside d_results was written"
        out = [res[FRONT:FRONT + n].copy(), None, None]
        if self.spans is not None:
            sp = self.spans.cpu().numpy().view(np.uint64)
            assert (sp[:8] == 0x0707070707070707).all() and (sp[8 + 2 * n + 1:] == 0x0707070707070707).all(), "a word outside d_spans was written"
            out[1] = sp[8:8 + 2 * n + 1].copy()
        if self.sres is not None:
            sr = self.sres.cpu().numpy()
            assert (sr[:FRONT] == 7).all() and (sr[FRONT + 2 * n:] == 7).all(), "a byte outside d_span_results was written"
            out[2] = sr[FRONT:FRONT + 2 * n].copy()
        return out

    def untouched(self):
        return bool((self.res == 7).all() and (self.spans is None or (self.spans == 0x0707070707070707).all())
                    and (self.sres is None or (self.sres == 7).all()))


def gpu_search(img, strings, exact=False, spans=True, span_results=True, stream=None):
    d_bytes, d_off, _ = testlib.upload(strings, exact)
    room = Room(len(strings), spans, span_results)
    img.search_tensors(d_bytes, d_off, *room.args(), stream=stream)
    torch.cuda.synchronize()
    return room.read()


def same(got, want, strings, what):
    res, spans, sres = got
    w_res, w_spans, w_sres = want
    bad = np.nonzero(res != w_res)[0]
    assert bad.size == 0, "%s: %d results differ, first line %d (len %d) want %d got %d" % (what, bad.size, bad[0], len(strings[bad[0]]), w_res[bad[0]], res[bad[0]])
    if spans is not None:
        bad = np.nonzero(spans != w_spans)[0]
        assert bad.size == 0, "%s: %d span words differ, first %d (line %d, len %d) want %d got %d" % (
            what, bad.size, bad[0], bad[0] // 2, len(strings[min(bad[0] // 2, len(strings) - 1)]), w_spans[bad[0]], spans[bad[0]])
    if sres is not None:
        assert np.array_equal(sres, w_sres), what


def parity_batch(name, blob, alpha, exe, tmp_path, k):
    """about 600 lines of 0 to 4097 bytes and one of 1 MiB whose only letters are its last bytes: a short line the harness finds a match
    in, behind a megabyte of z"""
    rng = np.random.default_rng(SEED + 2000 + k)
    strings = search_lib.long_strings(name, alpha, rng, count=600)
    probe = search_lib.short_strings(name, alpha, rng, count=60)
    res, _, _ = search_lib.emul_run(exe, blob, probe, tmp_path)
    tail = next((s for s, r in zip(probe, res) if r and s and b"z" not in s), b"")
    mib = b"z" * ((1 << 20) - len(tail)) + tail
    at = len(strings) // 2
    return strings[:at] + [mib] + strings[at:], at, len(tail)


NAMES = sorted(["%s_%s" % (n, d) for n in testlib.NFA_NAMES for d in ("fwd", "rev")] + ["table_66_fwd", "table_66_rev", "table_127_fwd", "table_127_rev", "ab5a_fwd"])


@pytest.mark.parametrize("name", NAMES)
def test_parity_with_the_harness(name, imgs, exe, tmp_path):
    blob, alpha = imgs[name]
    strings, at, tail = parity_batch(name, blob, alpha, exe, tmp_path, NAMES.index(name))
    want = search_lib.emul_run(exe, blob, strings, tmp_path)
    img = capi.Image(blob)
    same(gpu_search(img, strings), want, strings, name)
    assert img.info()["last_kernel"] == capi.KERNEL_SEARCH
    has_empty = bool(oracle_lib.OracleImage(blob).match([b""])[0])
    if tail and not has_empty:                                 # the megabyte's match lies in its last 100 bytes
        off = testlib.out_offsets(strings)
        assert want[0][at] == 1 and want[1][2 * at] >= off[at] + (1 << 20) - 100
    # results only: the second pass is not launched, the results are the same
    same(gpu_search(img, strings, spans=False, span_results=False), (want[0], None, None), strings, name + " results only")
    same(gpu_search(img, strings, span_results=False), want, strings, name + " without span results")
    img.close()


def test_both_forms_of_pass_one(imgs):
    """the fixtures' tables are tiled; table_66 reversed (66 sets) and table_127 reversed walk untiled"""
    tile = 4 * 64 * 144
    for name, (blob, _) in imgs.items():
        img = capi.Image(blob)
        s1, s2 = img.search_info()
        tiled = s1 * 258 * 2 + tile <= 65536
        assert tiled == (name not in ("table_66_rev", "table_127_rev", "ab5a_fwd")), (name, s1, s2)
        img.close()


@pytest.mark.parametrize("name", ["nfa_abb_thompson_fwd", "nfa_abb_thompson_rev", "table_66_fwd", "table_66_rev"])
def test_exact_room(name, imgs, exe, tmp_path):
    """the batch in exactly the room the read rule asks for, whole 16-byte blocks: both forms of pass 1, and pass 2"""
    blob, alpha = imgs[name]
    strings = search_lib.long_strings(name, alpha, np.random.default_rng(SEED + 7), count=600)
    want = search_lib.emul_run(exe, blob, strings, tmp_path)
    img = capi.Image(blob)
    same(gpu_search(img, strings, exact=True), want, strings, name)
    img.close()


def test_no_lines_and_empty_lines(imgs):
    img = capi.Image(imgs["nfa_abb_thompson_fwd"][0])
    res, spans, sres = gpu_search(img, [])
    assert res.size == 0 and list(spans) == [0] and sres.size == 0
    res, spans, sres = gpu_search(img, [b"", b"", b"abb", b""])
    assert list(res) == [0, 0, 1, 0] and list(spans) == [0, 0, 0, 0, 0, 3, 3, 3, 3] and list(sres) == [0, 0, 0, 0, 1, 0, 0, 0]
    img.close()


@pytest.mark.parametrize("name", ["nfa_abb_thompson_fwd", "table_66_rev"])
def test_a_line_beyond_the_limit(name, imgs, exe, tmp_path):
    """MFA_MAX_STRING_BYTES + 1 bytes: answered 2 with an empty span at its begin, and not read; its neighbours as without it"""
    blob, alpha = imgs[name]
    rng = np.random.default_rng(SEED + 11)
    around = search_lib.long_strings(name, alpha, rng, count=100)
    at = len(around) // 2
    big = testlib.rnd(alpha, testlib.MAX_BYTES + 1, rng)
    w_res, w_spans, w_sres = search_lib.emul_run(exe, blob, around, tmp_path)
    strings = around[:at] + [big] + around[at:]
    img = capi.Image(blob)
    res, spans, sres = gpu_search(img, strings)
    begin = sum(len(s) for s in around[:at])
    assert res[at] == 2 and spans[2 * at] == spans[2 * at + 1] == begin and list(sres[2 * at:2 * at + 2]) == [2, 0]
    assert np.array_equal(np.delete(res, at), w_res) and np.array_equal(np.delete(sres, [2 * at, 2 * at + 1]), w_sres)
    rest = np.delete(spans, [2 * at, 2 * at + 1]).astype(np.int64)
    rest[2 * at:] -= len(big)
    assert np.array_equal(rest, w_spans.astype(np.int64))
    img.close()


def _lines(rng, n, top=60):
    """n lines over a, b and z without a newline, a third of them empty or all z"""
    out = []
    for k in range(n):
        ln = int(rng.integers(0, top + 1))
        out.append(b"z" * ln if k % 3 == 0 else testlib.rnd(b"abz", ln, rng))
    return out


def _abb(line):
    """the leftmost-longest match of (a|b)*abb in a line, in Python: [ab]* is greedy and gives back only as far as the last abb of the run"""
    return re.search(rb"[ab]*abb", line)


def test_spans_as_a_batch(imgs):
    """capi.select on (d_bytes, d_spans, d_span_results) with NEWLINE: every line's match, joined by newlines; indices // 2 the line numbers"""
    rng = np.random.default_rng(SEED + 13)
    lines = _lines(rng, 3000)
    d_bytes, d_off, _ = testlib.upload(lines)
    n = len(lines)
    d_spans = torch.zeros(2 * n + 1, dtype=torch.int64, device="cuda")
    d_sres = torch.zeros(2 * n, dtype=torch.uint8, device="cuda")
    img = capi.Image(imgs["nfa_abb_thompson_fwd"][0])
    img.search_tensors(d_bytes, d_off, None, d_spans, d_sres)
    out, out_off, out_ind, info = capi.select(d_bytes, d_spans, d_sres, capi.SELECT_NEWLINE)
    torch.cuda.synchronize()
    found = [(k, _abb(s)) for k, s in enumerate(lines)]
    found = [(k, m.group(0)) for k, m in found if m]
    assert 100 < len(found) < n - 100
    assert info["n_selected"] == len(found) and info["n_unanswered"] == 0
    assert out.cpu().numpy()[:info["n_bytes"]].tobytes() == b"".join(m + b"\n" for _, m in found)
    ind = out_ind.cpu().numpy()
    assert (ind % 2 == 0).all() and list(ind // 2) == [k for k, _ in found]
    img.close()


def test_round_trip_from_a_text(imgs):
    """a text through capi.split_text, the search, capi.select on the line results: the lines Python keeps (with INVERT: the others)"""
    rng = np.random.default_rng(SEED + 17)
    lines = _lines(rng, 2500)
    text = b"".join(s + b"\n" for s in lines)
    d_text = torch.zeros((len(text) + 15) // 16 * 16, dtype=torch.uint8, device="cuda")
    d_text[:len(text)] = torch.frombuffer(bytearray(text), dtype=torch.uint8)
    d_bytes, d_off, n, _ = capi.split_text(d_text[:len(text)], capi.SPLIT_LINES)
    assert n == len(lines)
    img = capi.Image(imgs["nfa_abb_thompson_rev"][0])         # the mirrored language, scanned from the end: bba(a|b)*
    d_res = img.search_tensors(d_bytes, d_off)
    for flags, keep in ((capi.SELECT_NEWLINE, True), (capi.SELECT_NEWLINE | capi.SELECT_INVERT, False)):
        out, _, out_ind, info = capi.select(d_bytes, d_off, d_res, flags)
        torch.cuda.synchronize()
        want = [k for k, s in enumerate(lines) if (re.search(rb"bba", s) is not None) == keep]
        assert 100 < len(want) < n - 100 and list(out_ind.cpu().numpy()) == want
        assert out.cpu().numpy()[:info["n_bytes"]].tobytes() == b"".join(lines[k] + b"\n" for k in want)
    img.close()


@pytest.mark.parametrize("name", ["nfa_abb_thompson_fwd", "table_66_rev"])
def test_stream_capture(name, imgs, exe, tmp_path):
    """both passes captured once on a stream that a warm call has used (the tables are on the device), replayed twice on other bytes"""
    blob, alpha = imgs[name]
    rng = np.random.default_rng(SEED + 19)
    first = search_lib.long_strings(name, alpha, rng, count=300)
    second = [testlib.rnd(alpha + b"z", len(s), rng) for s in first]
    d_bytes, d_off, _ = testlib.upload(first)
    room = Room(len(first))
    img = capi.Image(blob)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        img.search_tensors(d_bytes, d_off, *room.args())
    torch.cuda.synchronize()
    same(room.read(), search_lib.emul_run(exe, blob, first, tmp_path), first, name + " warm")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        img.search_tensors(d_bytes, d_off, *room.args())
    torch.cuda.synchronize()
    for strings in (second, first):
        data, _ = oracle_lib.pack(strings)
        d_bytes[:len(data)] = torch.from_numpy(data.copy()).cuda()
        for t in (room.res, room.spans, room.sres):
            t.fill_(7 if t.dtype == torch.uint8 else 0x0707070707070707)
        g.replay()
        torch.cuda.synchronize()
        same(room.read(), search_lib.emul_run(exe, blob, strings, tmp_path), strings, name + " replay")
    img.close()


def test_refusals_leave_the_outputs_alone(imgs, tmp_path, monkeypatch):
    """a memory automaton, a set-walk image, 514 state sets, a pass 1 table beyond 127 sets: MFA_ERR_UNSUPPORTED; the argument errors; on
    real device buffers, and nothing is written"""
    strings = [b"abb", b"zz", b"aabbz"]
    d_bytes, d_off, _ = testlib.upload(strings)
    room = Room(len(strings))
    d_res, d_spans, d_sres = room.args()
    L = capi.lib()
    call = lambda img, off=d_off.data_ptr(), res=d_res.data_ptr(), spans=d_spans.data_ptr(), sres=d_sres.data_ptr(), n=3: \
        L.mfa_search_batch(img._h if img is not None else None, d_bytes.data_ptr(), off, n, res, spans, sres, 0, None)
    refused = {"ex1_plain": capi.Image(image.blob_from_dump(oracle_lib.load_dump("ex1_plain")))}
    monkeypatch.setenv("MFA_NFA_SETWALK", "1")
    refused["setwalk"] = capi.Image(testlib.fixture_blob("nfa_abb_thompson"))
    monkeypatch.delenv("MFA_NFA_SETWALK")
    refused["t514"] = capi.Image(testlib.table_blob("t514", tmp_path))
    refused["ab8a"] = capi.Image(testlib.front_end_blob("(a|b)" * 8 + "a", tmp_path))
    for name, img in refused.items():
        assert call(img) == capi.ERR_UNSUPPORTED and call(img, n=0) == capi.ERR_UNSUPPORTED, name
    good = capi.Image(imgs["nfa_abb_thompson_fwd"][0])
    bad = capi.ERR_INVALID_ARG
    assert call(None) == bad and call(good, off=None) == bad and call(good, res=None) == bad and call(good, spans=None) == bad
    assert call(good, spans=d_spans.data_ptr() + 4) == bad
    torch.cuda.synchronize()
    assert room.untouched()
    # and the same buffers take a well-formed call
    assert call(good) == capi.OK
    torch.cuda.synchronize()
    res, spans, sres = room.read()
    assert list(res) == [1, 0, 1] and list(spans) == [0, 3, 3, 3, 5, 9, 10] and list(sres) == [1, 0, 0, 0, 1, 0]
    for img in list(refused.values()) + [good]:
        img.close()


def test_host_pointers(imgs, exe, tmp_path):
    """mfa_search_batch_host: offsets that do not begin at 0 come back as absolute spans"""
    blob, alpha = imgs["nfa_abb_thompson_fwd"]
    strings = search_lib.long_strings("nfa_abb_thompson_fwd", alpha, np.random.default_rng(SEED + 23), count=200)
    w_res, w_spans, w_sres = search_lib.emul_run(exe, blob, strings, tmp_path)
    data, off = oracle_lib.pack(strings)
    shifted = np.concatenate([np.frombuffer(b"abbabb!", dtype=np.uint8), data])
    img = capi.Image(blob)
    res, spans, sres = img.search_host(shifted, off + np.uint64(7))
    assert np.array_equal(res, w_res) and np.array_equal(spans, w_spans + np.uint64(7)) and np.array_equal(sres, w_sres)
    res, spans, sres = img.search_host(shifted, off + np.uint64(7), want_spans=False)
    assert np.array_equal(res, w_res) and spans is None and sres is None
    img.close()


@pytest.mark.parametrize("flags", [[], ["-all"]])
def test_command_line(flags, tmp_path):
    """`diploma -search-lines FILE`, `-v` and `-o` on a file of 2000 lines with empty lines and a last line without a newline: the
    header of `-match-lines`, then what Python keeps; a regex with memory ends with the library's message and exit status 1"""
    rng = np.random.default_rng(SEED + 29)
    lines = _lines(rng, 2000)
    lines[5:5] = [b"", b"abb", b"", b"zabbz"]
    (tmp_path / "lines.txt").write_bytes(b"\n".join(lines))   # (the last line has no newline behind it)
    run = lambda regex, args: subprocess.run([testlib.DIPLOMA] + args + flags, input=regex.encode() + b"\n", capture_output=True, cwd=tmp_path, timeout=120)
    match = run("(a|b)*abb", ["-match-lines", str(tmp_path / "lines.txt")])
    assert match.returncode == 0, match.stderr
    header = match.stdout[:len(match.stdout) - 2 * len(lines)]
    hits = [_abb(s) for s in lines]
    assert 100 < sum(m is not None for m in hits) < len(lines) - 100
    wants = {(): b"".join(s + b"\n" for s, m in zip(lines, hits) if m), ("-v",): b"".join(s + b"\n" for s, m in zip(lines, hits) if not m),
             ("-o",): b"".join(m.group(0) + b"\n" for m in hits if m)}
    for extra, want in wants.items():
        got = run("(a|b)*abb", ["-search-lines", str(tmp_path / "lines.txt")] + list(extra))
        assert got.returncode == 0 and got.stdout == header + want, (extra, got.stderr)
    both = run("(a|b)*abb", ["-search-lines", str(tmp_path / "lines.txt"), "-v", "-o"])
    assert both.returncode == 1
    memory = run("({a*}:1&1)*", ["-search-lines", str(tmp_path / "lines.txt")])
    assert memory.returncode == 1 and b"outside the limits" in memory.stderr
