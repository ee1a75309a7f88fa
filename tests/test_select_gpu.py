"""Batch to text on the GPU (csrc/select.hip behind mfa_select_count and mfa_select_write): every case of tests/select_lib.py through the
C-ABI, byte for byte against the rule in Python and against the host harness -- info record, offsets, indices and bytes -- with guard
bytes in front of and behind all three outputs; the round trip through the splitter, a stream capture, the argument errors on real
buffers, and the whole way from a text to the lines that matched: split on the device, matched by mfa_match_batch, selected, against
the goldens; the command line against `diploma -match-lines` on the same file.  The pure part is checked by tests/test_select_cpu.py."""
import os
import subprocess

import numpy as np
import pytest
import torch

import oracle_lib
from mfa_amd import capi, image
from select_lib import (INVERT, NEWLINE, all_cases, case, emul_results, expected_case, fill, info_dict)
from testlib import DIPLOMA, emul_exe

pytestmark = pytest.mark.gpu
GUARD, GUARD8, FRONT = 0x5a, 0x5a5a5a5a5a5a5a5a, 64


def upload(c):
    """the case's batch on the device: the strings in exactly the aligned 16-byte blocks they touch, d_bytes & 15 == src_shift.  Returns
    (tensors to keep alive, d_bytes as a raw pointer, d_offsets, d_results)"""
    first = (c.src_shift + int(c.off[0])) // 16 * 16
    last = (c.src_shift + int(c.off[-1]) + 15) // 16 * 16
    blocks = torch.full((max(last - first, 16),), 0xa5, dtype=torch.uint8, device="cuda")
    if c.data:
        at = c.src_shift + int(c.off[0]) - first
        blocks[at:at + len(c.data)] = torch.frombuffer(bytearray(c.data), dtype=torch.uint8)
    d_off = torch.from_numpy(np.asarray(c.off, dtype=np.uint64).view(np.int64).copy()).to("cuda")
    d_res = torch.from_numpy(np.concatenate([np.asarray(c.res, dtype=np.uint8), np.zeros(1, dtype=np.uint8)])).to("cuda")
    assert blocks.data_ptr() % 16 == 0
    return (blocks,), blocks.data_ptr() - first + c.src_shift, d_off, d_res


class Room:
    """the three outputs of a case with guards in front of and behind each, the workspace and the info record"""

    def __init__(self, c):
        n = len(c.res)
        self.c = c
        self.work = torch.empty(max(capi.select_workspace_bytes(n), 16), dtype=torch.uint8, device="cuda")
        self.info = torch.full((4,), -1, dtype=torch.int64, device="cuda")
        self.bytes = torch.full((FRONT + c.dst_shift + c.capacity + 64,), GUARD, dtype=torch.uint8, device="cuda")
        self.off = torch.full((8 + c.max_selected + 1 + 8,), GUARD8, dtype=torch.int64, device="cuda")
        self.ind = torch.full((8 + c.max_selected + 8,), GUARD8, dtype=torch.int64, device="cuda")
        assert self.bytes.data_ptr() % 16 == 0
        self.p_bytes = self.bytes.data_ptr() + FRONT + c.dst_shift
        self.p_off = self.off.data_ptr() + 64
        self.p_ind = self.ind.data_ptr() + 64 if c.with_indices else None

    def read(self):
        """(the 32 bytes of the info, out_offsets[0..v], out_indices[0..v) or None, the bytes up to min(out_offsets[v], capacity)), after
        the guards have been looked at"""
        c = self.c
        raw_info = self.info.cpu().numpy().tobytes()
        host_bytes, host_off, host_ind = self.bytes.cpu().numpy(), self.off.cpu().numpy().view(np.uint64), self.ind.cpu().numpy().view(np.uint64)
        lo = FRONT + c.dst_shift
        assert (host_bytes[:lo] == GUARD).all() and (host_bytes[lo + c.capacity:] == GUARD).all(), "%s: a byte outside d_out_bytes was written" % c.name
        assert (host_off[:8] == GUARD8).all() and (host_off[8 + c.max_selected + 1:] == GUARD8).all(), "%s: an offset outside its array was written" % c.name
        assert (host_ind[:8] == GUARD8).all() and (host_ind[8 + c.max_selected:] == GUARD8).all(), "%s: an index outside its array was written" % c.name
        if not c.with_indices:
            assert (host_ind == GUARD8).all()
        v = min(info_dict(raw_info)["n_selected"], c.max_selected)
        off = host_off[8:8 + v + 1].copy()
        return raw_info, off, host_ind[8:8 + v].copy() if c.with_indices else None, host_bytes[lo:lo + min(int(off[v]), c.capacity)].tobytes()

    def untouched(self):
        return bool((self.bytes == GUARD).all() and (self.off == GUARD8).all() and (self.ind == GUARD8).all() and (self.info == -1).all())


def gpu_select(c):
    """count and write enqueued back to back on the current stream, nothing read back in between"""
    keep, p_bytes, d_off, d_res = upload(c)
    room = Room(c)
    s = torch.cuda.current_stream().cuda_stream
    n = len(c.res)
    capi.select_count(d_res.data_ptr(), d_off.data_ptr(), n, c.flags, room.work.data_ptr(), room.info.data_ptr(), 0, s)
    capi.select_write(p_bytes, d_off.data_ptr(), d_res.data_ptr(), n, c.flags, room.work.data_ptr(), room.info.data_ptr(),
                      room.p_bytes if c.capacity else None, c.capacity, room.p_off, room.p_ind, c.max_selected, 0, s)
    torch.cuda.synchronize()
    return room.read()


def same(got, want_py, want_emul, c):
    raw_info, off, ind, data = got
    w_info, w_off, w_ind, w_data = want_py
    assert info_dict(raw_info) == w_info, c.name
    assert np.array_equal(off, w_off), c.name
    assert ind is None or np.array_equal(ind, w_ind), c.name
    assert data == w_data, c.name
    if want_emul is not None:
        e_info, e_off, e_ind, e_data = want_emul
        assert raw_info == e_info and np.array_equal(off, e_off) and data == e_data and (ind is None or np.array_equal(ind, e_ind)), c.name


def test_every_case_against_python_and_the_harness(tmp_path):
    """degenerate counts, string lengths, every alignment pair, the borders of the count block and one n beyond a round of the scan
    workgroup, every clipping and the 200 random batches: count and write with no wait in between, compared with the rule in Python and,
    byte for byte, with what the host harness leaves"""
    cases = all_cases()
    emul = emul_results(emul_exe("select"), tmp_path, cases)
    for c, e in zip(cases, emul):
        same(gpu_select(c), expected_case(c), e, c)


def test_no_wait_order():
    """count and write back to back with sizes the caller bounds itself (n strings, offsets[n] - offsets[0] + n bytes): no read-back, no
    overflow, and the counts arrive with the output"""
    strings = [fill(k % 50, k) for k in range(3000)]
    c = case("no_wait", strings, [k % 3 == 0 for k in range(3000)], NEWLINE, off0=7, dst_shift=3)
    assert c.max_selected == 3000 and c.capacity == sum(len(s) for s in strings) + 3000
    got = gpu_select(c)
    same(got, expected_case(c), None, c)
    assert info_dict(got[0])["overflow"] == 0 and info_dict(got[0])["n_selected"] == 1000


def test_round_trip_through_the_splitter():
    """lines without 0x0a, all kept, NEWLINE: a text that capi.split_text in lines mode cuts back into the same bytes and offsets"""
    strings = [fill((7 * k) % 90, k) for k in range(2500)] + [b"", fill(40000, 3), b""]
    data = b"".join(strings)
    off = np.zeros(len(strings) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(s) for s in strings])
    d_bytes = torch.zeros((len(data) + 15) // 16 * 16, dtype=torch.uint8, device="cuda")
    d_bytes[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    d_off = torch.from_numpy(off).to("cuda")
    d_res = torch.ones(len(strings), dtype=torch.uint8, device="cuda")
    text, out_off, out_ind, info = capi.select(d_bytes, d_off, d_res, capi.SELECT_NEWLINE)
    assert info["n_selected"] == len(strings) and info["n_bytes"] == len(data) + len(strings) and info["n_unanswered"] == 0
    assert np.array_equal(out_ind.cpu().numpy(), np.arange(len(strings))) and int(info["d_info"].cpu()[3]) == 0
    assert text.cpu().numpy()[:info["n_bytes"]].tobytes() == b"".join(s + b"\n" for s in strings)
    back_bytes, back_off, n, back = capi.split_text(text[:info["n_bytes"]], capi.SPLIT_LINES)
    torch.cuda.synchronize()
    assert n == len(strings) and back["n_bytes"] == len(data)
    assert np.array_equal(back_off.cpu().numpy(), off) and back_bytes.cpu().numpy()[:len(data)].tobytes() == data


def test_stream_capture():
    """count + write captured once on one stream (a linear chain of launches) and replayed on changed result bytes"""
    strings = [fill(k % 37, k) for k in range(2100)]
    c = case("capture", strings, [k % 2 for k in range(2100)], NEWLINE, dst_shift=4)
    keep, p_bytes, d_off, d_res = upload(c)
    room = Room(c)
    n = len(c.res)
    gpu_select(c)                                             # (the kernels are loaded before the capture begins)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s = torch.cuda.current_stream().cuda_stream
        capi.select_count(d_res.data_ptr(), d_off.data_ptr(), n, c.flags, room.work.data_ptr(), room.info.data_ptr(), 0, s)
        capi.select_write(p_bytes, d_off.data_ptr(), d_res.data_ptr(), n, c.flags, room.work.data_ptr(), room.info.data_ptr(), room.p_bytes, c.capacity,
                          room.p_off, room.p_ind, c.max_selected, 0, s)
    for results in ([k % 2 for k in range(2100)], [k % 5 == 0 for k in range(2100)], [0] * 2100):
        d_res[:n] = torch.tensor(results, dtype=torch.uint8, device="cuda")
        graph.replay()
        torch.cuda.synchronize()
        now = c._replace(res=np.asarray(results, dtype=np.uint8))
        same(room.read(), expected_case(now), None, now)


def test_argument_errors_leave_the_outputs_alone():
    """every MFA_ERR_INVALID_ARG of the contract on real device buffers: refused, and nothing written"""
    c = case("errors", [fill(20, k) for k in range(10)], [1] * 10)
    keep, p_bytes, d_off, d_res = upload(c)
    room = Room(c)
    L = capi.lib()
    n, bad = 10, capi.ERR_INVALID_ARG
    good_count = dict(results=d_res.data_ptr(), offsets=d_off.data_ptr(), n=n, flags=0, work=room.work.data_ptr(), info=room.info.data_ptr())
    good_write = dict(good_count, src=p_bytes, out=room.p_bytes, cap=c.capacity, off=room.p_off, ind=room.p_ind, ms=c.max_selected)
    count = lambda a: L.mfa_select_count(a["results"], a["offsets"], a["n"], a["flags"], a["work"], a["info"], 0, None)
    write = lambda a: L.mfa_select_write(a["src"], a["offsets"], a["results"], a["n"], a["flags"], a["work"], a["info"], a["out"], a["cap"], a["off"], a["ind"],
                                         a["ms"], 0, None)
    for key in ("results", "offsets", "work", "info"):
        assert count(dict(good_count, **{key: None})) == bad and write(dict(good_write, **{key: None})) == bad, key
    for key in ("src", "out", "off"):
        assert write(dict(good_write, **{key: None})) == bad, key
    for flags in (4, 0x10, 0xfffffffc):
        assert count(dict(good_count, flags=flags)) == bad and write(dict(good_write, flags=flags)) == bad
    assert count(dict(good_count, work=good_count["work"] + 8)) == bad and write(dict(good_write, work=good_write["work"] + 8)) == bad
    for key in ("info", "offsets"):
        assert count(dict(good_count, **{key: good_count[key] + 4})) == bad and write(dict(good_write, **{key: good_write[key] + 4})) == bad, key
    for key in ("off", "ind"):
        assert write(dict(good_write, **{key: good_write[key] + 4})) == bad, key
    assert count(dict(good_count, n=1 << 40)) == bad and write(dict(good_write, n=1 << 40)) == bad
    torch.cuda.synchronize()
    assert room.untouched()
    # and the same buffers take a well-formed pair of calls
    assert count(good_count) == capi.OK and write(good_write) == capi.OK
    torch.cuda.synchronize()
    same(room.read(), expected_case(c), None, c)


def golden_text(name):
    strings = [s for s in oracle_lib.load_set("abc7") if b"\n" not in s]
    bits = np.array([b for s, b in zip(oracle_lib.load_set("abc7"), oracle_lib.load_bits(name, "abc7")) if b"\n" not in s], dtype=np.uint8)
    assert len(strings) > 1000
    return strings, bits, b"".join(s + b"\n" for s in strings)


@pytest.mark.parametrize("name", ["nfa_abb_plain", "ex1_plain"])
def test_text_to_matching_lines(name):
    """the golden strings joined by newlines: split on the device, matched where they lie, selected with NEWLINE -- the golden-accepted
    lines joined in Python; with INVERT the golden-rejected ones"""
    strings, bits, text = golden_text(name)
    d_text = torch.zeros((len(text) + 15) // 16 * 16, dtype=torch.uint8, device="cuda")
    d_text[:len(text)] = torch.frombuffer(bytearray(text), dtype=torch.uint8)
    d_bytes, d_off, n, _ = capi.split_text(d_text[:len(text)], capi.SPLIT_LINES)
    assert n == len(strings)
    d_res = capi.Image(image.blob_from_dump(oracle_lib.load_dump(name))).match_tensors(d_bytes, d_off)
    for flags, keep in ((capi.SELECT_NEWLINE, 1), (capi.SELECT_NEWLINE | capi.SELECT_INVERT, 0)):
        out, out_off, out_ind, info = capi.select(d_bytes, d_off, d_res, flags)
        torch.cuda.synchronize()
        want = [s for s, b in zip(strings, bits) if b == keep]
        assert info["n_selected"] == len(want) and info["n_unanswered"] == 0
        assert out.cpu().numpy()[:info["n_bytes"]].tobytes() == b"".join(s + b"\n" for s in want)
        assert np.array_equal(out_ind.cpu().numpy(), np.nonzero(bits == keep)[0])


@pytest.mark.parametrize("regex,flags", [("(a|b)*abb", []), ("({a*}:1&1)*", []), ("(a|b)*abb", ["-all"])])
def test_command_line(regex, flags, tmp_path):
    """`diploma -grep-lines FILE` and `-grep-lines FILE -v` on a file of a few hundred lines with empty lines, \\r and a last line without
    a newline: the header of `-match-lines`, then the lines it answered 1 (0 with -v); DIPLOMA_DEVICE_SELECT=0 prints the same"""
    lines = [s for s in oracle_lib.load_set("abc7") if b"\n" not in s][:400]
    lines[5:5] = [b"", b"abb\r", b"", b""]
    lines += [b"aabb\r", b"", b"babb"]
    body = b"\n".join(lines)                                  # (the last line has no newline behind it)
    (tmp_path / "lines.txt").write_bytes(body)
    env = {k: v for k, v in os.environ.items() if k not in ("DIPLOMA_DEVICE_SELECT", "DIPLOMA_DEVICE_SPLIT")}
    run = lambda args, env: subprocess.run([DIPLOMA] + args + flags, input=regex.encode() + b"\n", capture_output=True, cwd=tmp_path, env=env, timeout=120)
    match = run(["-match-lines", str(tmp_path / "lines.txt")], env)
    assert match.returncode == 0, match.stderr
    answers = match.stdout.split(b"\n")[-len(lines) - 1:-1]
    assert set(answers) == {b"0", b"1"} and match.stdout.endswith(b"\n")
    header = match.stdout[:len(match.stdout) - 2 * len(lines)]
    for extra, keep in (([], b"1"), (["-v"], b"0")):
        want = header + b"".join(s + b"\n" for s, a in zip(lines, answers) if a == keep)
        got = run(["-grep-lines", str(tmp_path / "lines.txt")] + extra, env)
        assert got.returncode == 0 and got.stdout == want, got.stderr
        host = run(["-grep-lines", str(tmp_path / "lines.txt")] + extra, dict(env, DIPLOMA_DEVICE_SELECT="0"))
        assert host.returncode == 0 and host.stdout == want, host.stderr
