"""What tests/test_text_split_cpu.py and tests/test_text_split_gpu.py share: the rule in Python, the case files of the host harness
tests/emul/text_split_emul.cpp (built by testlib.emul_exe) and its output, the edge texts and the seeded random ones --
TEST INFRASTRUCTURE ONLY: no tests, no fixtures, no marks in here."""
import os
import struct
import subprocess

import numpy as np

from testlib import CSRC

LINES, TOKENS = 0, 1
STOP = b"exit"
ALPHABET = [b"a", b"b", b"e", b"x", b"i", b"t", b" ", b"\n", b"\t", b"\r", b"\x0b", b"\x00"]


def tile_bytes():
    """kSplitTileBytes of csrc/text_split_core.h, as the harness was compiled with it (the library's mfa_split_tile_bytes() must agree)"""
    import re
    with open(os.path.join(CSRC, "text_split_core.h")) as f:
        src = f.read()
    threads = int(re.search(r"kSplitThreads = (\d+)u", src).group(1))
    rows = int(re.search(r"kSplitRows = (\d+)u", src).group(1))
    return threads * rows * 16


# ---- the rule, in Python ----------------------------------------------------------------------------------------------------------------
def py_split(text, mode, stop=None):
    """(strings, stopped): bytes.split() for tokens, cut in front of the first token equal to `stop`; split(b"\\n") minus a trailing empty
    element for lines"""
    if mode == LINES:
        parts = text.split(b"\n")
        if parts[-1] == b"":
            parts.pop()
        return parts, False
    parts = text.split()
    if stop is not None and stop in parts:
        return parts[:parts.index(stop)], True
    return parts, False


def expected(text, mode, stop=None, max_strings=None, capacity=None):
    """what a count and a write must leave: (info dict, offsets[0..v], bytes[0..min(offsets[v], capacity)))"""
    strings, stopped = py_split(text, mode, stop)
    off = np.zeros(len(strings) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in strings], dtype=np.uint64)
    data = b"".join(strings)
    max_strings = len(strings) if max_strings is None else max_strings
    capacity = len(data) if capacity is None else capacity
    v = min(len(strings), max_strings)
    info = {"n_strings": len(strings), "n_bytes": len(data), "max_string_bytes": max([len(s) for s in strings[:v]], default=0),
            "stopped": int(stopped), "overflow": int(len(strings) > max_strings or len(data) > capacity)}
    return info, off[:v + 1], data[:min(int(off[v]), capacity)]


# ---- the harness ------------------------------------------------------------------------------------------------------------------------
INFO = struct.Struct("<QQQII")


def info_dict(raw):
    return dict(zip(("n_strings", "n_bytes", "max_string_bytes", "stopped", "overflow"), INFO.unpack(raw)))


def write_cases(path, cases):
    """CASES.bin of the harness; a case is (text, mode, stop or None, max_strings or None, capacity or None) -- None: room for everything"""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for text, mode, stop, max_strings, capacity in cases:
            stop = stop or b""
            f.write(struct.pack("<II16sQQQ", mode, len(stop), stop, len(text) + 1 if max_strings is None else max_strings,
                                len(text) if capacity is None else capacity, len(text)))
            f.write(text)


def parse_emul(raw, cases):
    """the harness's output for `cases`: a list of (info dict, offsets[0..v], the bytes written: min(offsets[v], capacity) of them, the 32 raw
    bytes of the info)"""
    out, at = [], 0
    for text, mode, stop, max_strings, capacity in cases:
        info = raw[at:at + 32]
        v = struct.unpack_from("<Q", raw, at + 32)[0]
        off = np.frombuffer(raw, dtype="<u8", count=v + 1, offset=at + 40)
        at += 40 + 8 * (v + 1)
        n_out = min(int(off[v]), len(text) if capacity is None else capacity)
        out.append((info_dict(info), off, raw[at:at + n_out], info))
        at += n_out
    assert at == len(raw)
    return out


def emul_results(exe, tmp_path, cases):
    write_cases(tmp_path / "cases.bin", cases)
    p = subprocess.run([exe, str(tmp_path / "cases.bin")], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()[-800:]
    return parse_emul(p.stdout, cases)


# ---- texts ------------------------------------------------------------------------------------------------------------------------------
def edge_texts(T):
    """name -> text: the edge list of the rule and the borders of a tile (T bytes), a wave's row (1024) and a block (16)"""
    fill = lambda n: (b"abxt" * (n // 4 + 1))[:n]
    out = {"empty": b"", "newline": b"\n", "a_nl_b": b"a\nb", "a_nl_b_nl": b"a\nb\n", "cr_nul": b"a\r\n\x00b\n\n\nc", "blank_lines": b"\n\n\n",
           "only_seps": b" \t\n\r\x0b\x0c" * 700, "no_sep": fill(3000), "high_bytes": bytes(range(256)) * 3,
           "long_string": fill(2 * T + 700) + b"\n" + fill(5), "long_first": b"ab " + fill(2 * T + 9),
           "sep_run_over_tile": fill(T - 3) + b" \n\t \n " + fill(40), "token_over_tile": fill(T - 9) + b" " + fill(20) + b"\nzz",
           "token_over_wave": fill(1000) + b" " + fill(60) + b" q", "token_over_block": b"abc " + fill(20) + b"\nq",
           "nl_last_of_tile": fill(T - 1) + b"\n" + fill(7), "nl_first_of_next": fill(T) + b"\n" + fill(7),
           "nl_both": fill(T - 1) + b"\n\n" + fill(7),
           "stop_over_tile": fill(T - 5) + b" b ex" + b"it c d", "stop_sep_in_next_tile": fill(T - 7) + b" b exit c d", "stop_first_of_two": b"a b exit c exit d", "stop_first_token": b"exit a b",
           "stop_first_token_sep": b"  exit a b", "stop_last_no_sep": b"a b exit", "stop_not": b"exits xexit ex it exi", "stop_then_not": b"xexit exits exit q",
           "stop_at_tile_end": fill(T - 5) + b" exit", "stop_at_tile_start": fill(T - 1) + b" exit\nq", "stop_in_third_tile": (fill(50) + b"\n") * (2 * T // 51 + 3) + b"exit " + fill(99),
           "stop_prefix_at_end": b"a exi", "stop_long_tail": b"a exit" + fill(30)}
    for n in (0, 1, 15, 16, 17, 1023, 1024, 1025, T - 1, T, T + 1, 2 * T + 1):
        out["len_%d" % n] = (b"ab cd\nef\tg  " * (n // 12 + 1))[:n]
        out["len_%d_nosep" % n] = fill(n)
    return out


def random_texts(T, count=300, seed=20261020):
    """`count` seeded texts of 0 to 5 tiles over ALPHABET; every third thins the separators out, so that strings cross blocks, rows and tiles"""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"".join(ALPHABET), dtype=np.uint8)
    out = []
    for k in range(count):
        n = int(rng.integers(0, 5 * T + 1))
        if k % 3 == 0:
            w = np.ones(len(letters))
        else:
            w = np.array([1.0] * 6 + [0.02 if k % 3 == 1 else 0.002] * 5 + [0.3])
        text = letters[rng.choice(len(letters), size=n, p=w / w.sum())].tobytes()
        if k % 5 == 2 and n > 40:                           # a stop token for certain, somewhere
            at = int(rng.integers(0, n - 6))
            text = text[:at] + b" exit " + text[at + 6:]
        out.append(text)
    return out


def both_modes(texts):
    """every text as a lines case and as a tokens case with the stop token, room for everything"""
    return [(t, LINES, None, None, None) for t in texts] + [(t, TOKENS, STOP, None, None) for t in texts]
