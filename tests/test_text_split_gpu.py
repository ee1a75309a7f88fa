"""Text to batch on the GPU (csrc/text_split.hip behind mfa_split_text_count and mfa_split_text_write): every case in both modes
against the rule in Python, the 300 random texts of the CPU test byte for byte against the host harness, guard bytes behind both
capacities, and the whole way from a text to answers: split on the device, matched by mfa_match_batch, against the goldens; the command
line against `diploma -match` on the same tokens.  The pure part is checked by tests/test_text_split_cpu.py."""
import os
import subprocess

import numpy as np
import pytest
import torch

import oracle_lib
from mfa_amd import capi, image
from testlib import DIPLOMA, emul_exe
from textsplit_lib import (LINES, STOP, TOKENS, both_modes, edge_texts, emul_results, expected, info_dict, py_split, random_texts)

pytestmark = pytest.mark.gpu
GUARD = 0x5a


@pytest.fixture(scope="module")
def T():
    return capi.split_tile_bytes()


def on_device(text):
    """the text in exactly the room the read rule asks for: its size rounded up to 16 (at least 16), 16-byte aligned"""
    d = torch.zeros(max((len(text) + 15) // 16 * 16, 16), dtype=torch.uint8, device="cuda")
    if text:
        d[:len(text)] = torch.frombuffer(bytearray(text), dtype=torch.uint8)
    return d


def gpu_split(text, mode, stop=None, max_strings=None, capacity=None, shift=0):
    """count and write with no read-back in between: room for max_strings strings (default: as many as the text can hold) and `capacity`
    bytes (default: the text's size), then 64 guard bytes and 8 guard offsets behind them; d_bytes starts `shift` bytes off a 16-byte line.
    Returns (the 32 bytes of the info, offsets[0..v], the bytes written up to min(offsets[v], capacity))"""
    max_strings = len(text) + 1 if max_strings is None else max_strings
    capacity = len(text) if capacity is None else capacity
    d_text = on_device(text)
    work = torch.empty(max(capi.split_workspace_bytes(len(text)), 16), dtype=torch.uint8, device="cuda")
    d_info = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    room = torch.full((shift + capacity + 64,), GUARD, dtype=torch.uint8, device="cuda")
    d_off = torch.full((max_strings + 1 + 8,), 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    capi.split_text_count(d_text.data_ptr(), len(text), mode, stop, work.data_ptr(), d_info.data_ptr(), 0, s)
    capi.split_text_write(d_text.data_ptr(), len(text), mode, work.data_ptr(), d_info.data_ptr(), room.data_ptr() + shift, capacity, d_off.data_ptr(),
                          max_strings, 0, s)
    torch.cuda.synchronize()
    raw_info = d_info.cpu().numpy().tobytes()
    info = info_dict(raw_info)
    host_room, host_off = room.cpu().numpy(), d_off.cpu().numpy().view(np.uint64)
    assert (host_room[:shift] == GUARD).all() and (host_room[shift + capacity:] == GUARD).all(), "a byte outside d_bytes was written"
    assert (host_off[max_strings + 1:] == 0x5a5a5a5a5a5a5a5a).all(), "an offset above max_strings was written"
    v = min(info["n_strings"], max_strings)
    off = host_off[:v + 1].copy()
    return raw_info, off, host_room[shift:shift + min(int(off[v]), capacity)].tobytes()


def check_against_python(text, mode, stop, what, max_strings=None, capacity=None, shift=0):
    max_strings = len(text) + 1 if max_strings is None else max_strings
    capacity = len(text) if capacity is None else capacity
    raw_info, off, data = gpu_split(text, mode, stop, max_strings, capacity, shift)
    w_info, w_off, w_data = expected(text, mode, stop, max_strings, capacity)
    assert info_dict(raw_info) == w_info, what
    assert np.array_equal(off, w_off), what
    assert data == w_data, what
    return info_dict(raw_info)


def test_lengths_and_placements(T):
    """lengths around a block, a wave's row and a tile; only separators and none; a string of more than two tiles; separators, tokens and
    newlines on the borders -- lines, tokens, and tokens with the stop token"""
    for k, (name, text) in enumerate(edge_texts(T).items()):
        for mode, stop in ((LINES, None), (TOKENS, None), (TOKENS, STOP)):
            check_against_python(text, mode, stop, "%s mode %d stop %s" % (name, mode, stop), shift=k % 16)


def test_stop_token(T):
    texts = edge_texts(T)
    for name in [n for n in texts if n.startswith("stop_")]:
        info = check_against_python(texts[name], TOKENS, STOP, name)
        assert info["stopped"] == int(name not in ("stop_not", "stop_prefix_at_end", "stop_long_tail")), name
    for stop in (b"q", b"123456789", b"123456789abcdef", b"\xff\x80z"):
        text = b"a " + stop + b"x y" + stop + b" " + stop[:-1] + b" " + (b"ab " * 6000)[:T - 40] + b" " + stop
        assert check_against_python(text, TOKENS, stop, repr(stop))["stopped"] == 1
        assert check_against_python(text[:-1], TOKENS, stop, repr(stop))["stopped"] == 0


def test_random_texts_against_the_harness(T, tmp_path):
    """the 300 random texts of the CPU test, both modes: info record, offsets and bytes as the host harness leaves them, byte for byte"""
    cases = both_modes(random_texts(T))
    want = emul_results(emul_exe("text_split"), tmp_path, cases)
    for k, ((text, mode, stop, _, _), (_, w_off, w_data, w_raw)) in enumerate(zip(cases, want)):
        raw_info, off, data = gpu_split(text, mode, stop, shift=k % 16)
        assert raw_info == w_raw, "case %d: %r != %r" % (k, info_dict(raw_info), info_dict(w_raw))
        assert np.array_equal(off, w_off) and data == w_data, "case %d" % k


def test_guards_and_overflow(T):
    """capacities that are too small, one and both: nothing outside them is touched (gpu_split checks the guards), overflow is 1, the
    counts are the true ones, and what fits is right; with exact room overflow is 0"""
    texts = random_texts(T, count=8, seed=7) + [edge_texts(T)["long_string"], b"a b c"]
    for k, text in enumerate(texts):
        for mode, stop in ((LINES, None), (TOKENS, STOP)):
            strings, _ = py_split(text, mode, stop)
            n, nb = len(strings), sum(len(s) for s in strings)
            for max_strings, capacity in ((n // 2, nb), (n, nb // 2), (n // 3, nb // 3), (0, 0), (n, nb), (max(n, 1) - 1, max(nb - 1, 0))):
                info = check_against_python(text, mode, stop, "text %d mode %d room %d/%d" % (k, mode, max_strings, capacity),
                                            max_strings=max_strings, capacity=capacity, shift=(3 * k + 1) % 16)
                assert info["overflow"] == int(max_strings < n or capacity < nb) and (info["n_strings"], info["n_bytes"]) == (n, nb)


def golden_text(name):
    strings = [s for s in oracle_lib.load_set("abc7") if b"\n" not in s]
    bits = np.array([b for s, b in zip(oracle_lib.load_set("abc7"), oracle_lib.load_bits(name, "abc7")) if b"\n" not in s], dtype=np.uint8)
    assert len(strings) > 1000
    return strings, bits, b"".join(s + b"\n" for s in strings)


@pytest.mark.parametrize("name", ["nfa_abb_plain", "ex1_plain"])
def test_split_then_match(name):
    """the golden strings joined by newlines, split on the device by capi.split_text and matched where they lie: the goldens' answers"""
    strings, bits, text = golden_text(name)
    d_bytes, d_off, n, info = capi.split_text(on_device(text)[:len(text)], capi.SPLIT_LINES)
    assert n == len(strings) and info["n_bytes"] == sum(len(s) for s in strings) and info["stopped"] == 0
    img = capi.Image(image.blob_from_dump(oracle_lib.load_dump(name)))
    got = img.match_tensors(d_bytes, d_off)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), bits)
    rest = [int(x) for x in info["d_info"].cpu()]
    assert rest[2] == max(len(s) for s in strings) and rest[3] == 0


@pytest.mark.parametrize("regex,flags", [("(a|b)*abb", []), ("({a*}:1&1)*", []), ("(a|b)*abb", ["-all"])])
def test_command_line(regex, flags, tmp_path):
    """`diploma -match-lines FILE` and `DIPLOMA_DEVICE_SPLIT=1 diploma -match`: byte-identical to `diploma -match` on the same tokens"""
    tokens = [s for s in oracle_lib.load_set("abc7") if s and not any(c in s for c in b" \t\n\r\x0b\x0c") and s != b"exit"][:3000]
    assert len(tokens) > 1000
    body = b"".join(t + b"\n" for t in tokens)
    (tmp_path / "lines.txt").write_bytes(body)
    stdin = regex.encode() + b"\n" + body + b"exit\nnot matched any more\n"
    env = {k: v for k, v in os.environ.items() if k != "DIPLOMA_DEVICE_SPLIT"}
    run = lambda args, data, env: subprocess.run([DIPLOMA] + args + flags, input=data, capture_output=True, cwd=tmp_path, env=env, timeout=120)
    plain = run(["-match"], stdin, env)
    assert plain.returncode == 0 and plain.stdout.count(b"\n") >= len(tokens), plain.stderr
    split = run(["-match"], stdin, dict(env, DIPLOMA_DEVICE_SPLIT="1"))
    assert split.returncode == 0 and split.stdout == plain.stdout, split.stderr
    lines = run(["-match-lines", str(tmp_path / "lines.txt")], regex.encode() + b"\n", env)
    assert lines.returncode == 0 and lines.stdout == plain.stdout, lines.stderr
