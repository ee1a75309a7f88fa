"""What tests/test_select_cpu.py and tests/test_select_gpu.py share: the rule of the selection in Python, the case files of the host harness
tests/emul/select_emul.cpp (built by testlib.emul_exe) and its output, the edge cases and the seeded random ones --
TEST INFRASTRUCTURE ONLY: no tests, no fixtures, no marks in here."""
import collections
import os
import re
import struct
import subprocess

import numpy as np

from testlib import CSRC

INVERT, NEWLINE = 1, 2
ALL_FLAGS = (0, INVERT, NEWLINE, INVERT | NEWLINE)


def geometry():
    """(kSelectBlock, kSelectTileBytes, strings per round of the scan workgroup) of csrc/select_core.h and csrc/select.hip, as the harness
    and the library were compiled with them"""
    with open(os.path.join(CSRC, "select_core.h")) as f:
        core = f.read()
    with open(os.path.join(CSRC, "select.hip")) as f:
        hip = f.read()
    threads = int(re.search(r"kSelectThreads = (\d+)u", core).group(1))
    per_lane = int(re.search(r"kSelectPerLane = (\d+)u", core).group(1))
    per_thread = int(re.search(r"kSelectScanPerThread = (\d+)u", hip).group(1))
    return threads * per_lane, threads * per_lane * 16, threads * per_thread * threads * per_lane


# ---- a case -----------------------------------------------------------------------------------------------------------------------------
# data: the strings' bytes from offsets[0] on; off: uint64[n + 1]; res: uint8[n]; src_shift, dst_shift: d_bytes & 15 and d_out_bytes & 15;
# max_selected, capacity: the room of the outputs
Case = collections.namedtuple("Case", "name data off res flags src_shift dst_shift with_indices max_selected capacity")


def bound(off, flags):
    """what a caller who has read nothing back can say of the output: (at most n strings, at most offsets[n] - offsets[0] (+ n) bytes)"""
    n = len(off) - 1
    return n, int(off[n] - off[0]) + (n if flags & NEWLINE else 0)


def case(name, strings, results, flags=0, off0=0, src_shift=0, dst_shift=0, with_indices=1, max_selected=None, capacity=None):
    """a case from a list of strings; max_selected, capacity None: the caller's own bound"""
    off = np.zeros(len(strings) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in strings], dtype=np.uint64)
    return case_of(name, b"".join(strings), off + np.uint64(off0), np.asarray(results, dtype=np.uint8), flags, src_shift, dst_shift, with_indices,
                   max_selected, capacity)


def case_of(name, data, off, res, flags=0, src_shift=0, dst_shift=0, with_indices=1, max_selected=None, capacity=None):
    assert len(res) == len(off) - 1 and len(data) == int(off[-1] - off[0])
    n, nb = bound(off, flags)
    return Case(name, data, off, res, flags, src_shift, dst_shift, with_indices, n if max_selected is None else max_selected,
                nb if capacity is None else capacity)


# ---- the rule, in Python ----------------------------------------------------------------------------------------------------------------
def expected(data, off, res, flags, max_selected, capacity):
    """what a count and a write must leave: (info dict, out_offsets[0..v], out_indices[0..v), out_bytes[0..min(out_offsets[v], capacity))).
    data: the bytes from offsets[0] on -- string k is data[off[k] - off[0] : off[k + 1] - off[0]]"""
    off = np.asarray(off, dtype=np.uint64).astype(np.int64)
    res = np.asarray(res, dtype=np.uint8)
    nl = 1 if flags & NEWLINE else 0
    kept = res == (0 if flags & INVERT else 1)
    idx = np.nonzero(kept)[0]
    lens = (off[1:] - off[:-1])[idx]
    out_off = np.zeros(len(idx) + 1, dtype=np.int64)
    out_off[1:] = np.cumsum(lens + nl)
    total = int(out_off[-1])
    raw = np.frombuffer(data, dtype=np.uint8)
    # output position p of string r comes from data[start[r] + p - out_off[r]]; the position behind a string is its newline
    src = np.repeat(off[:-1][idx] - off[0] - out_off[:-1], lens + nl) + np.arange(total, dtype=np.int64)
    out = raw[np.minimum(src, max(len(raw) - 1, 0))].copy() if len(raw) else np.zeros(total, dtype=np.uint8)
    if nl:
        out[out_off[1:] - 1] = 0x0a
    v = min(len(idx), max_selected)
    info = {"n_selected": len(idx), "n_bytes": total, "n_unanswered": int((res > 1).sum()),
            "overflow": int(len(idx) > max_selected or total > capacity), "reserved": 0}
    return info, out_off[:v + 1].astype(np.uint64), idx[:v].astype(np.uint64), out[:min(int(out_off[v]), capacity)].tobytes()


def expected_case(c):
    return expected(c.data, c.off, c.res, c.flags, c.max_selected, c.capacity)


# ---- the harness ------------------------------------------------------------------------------------------------------------------------
INFO = struct.Struct("<QQQII")


def info_dict(raw):
    return dict(zip(("n_selected", "n_bytes", "n_unanswered", "overflow", "reserved"), INFO.unpack(raw)))


def write_cases(path, cases):
    """CASES.bin of the harness"""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c in cases:
            f.write(struct.pack("<IIIIQQQ", c.flags, c.src_shift, c.dst_shift, c.with_indices, c.max_selected, c.capacity, len(c.res)))
            f.write(np.asarray(c.off, dtype="<u8").tobytes())
            f.write(np.asarray(c.res, dtype=np.uint8).tobytes())
            f.write(c.data)


def parse_emul(raw, cases):
    """the harness's output for `cases`: a list of (the 32 raw bytes of the info, out_offsets[0..v], out_indices[0..v) or None, the bytes
    written: min(out_offsets[v], capacity) of them)"""
    out, at = [], 0
    for c in cases:
        info = raw[at:at + 32]
        v = struct.unpack_from("<Q", raw, at + 32)[0]
        off = np.frombuffer(raw, dtype="<u8", count=v + 1, offset=at + 40)
        at += 40 + 8 * (v + 1)
        ind = None
        if c.with_indices:
            ind = np.frombuffer(raw, dtype="<u8", count=v, offset=at)
            at += 8 * v
        n_out = min(int(off[v]), c.capacity)
        out.append((info, off, ind, raw[at:at + n_out]))
        at += n_out
    assert at == len(raw)
    return out


def emul_results(exe, tmp_path, cases):
    write_cases(tmp_path / "select_cases.bin", cases)
    p = subprocess.run([exe, str(tmp_path / "select_cases.bin")], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()[-800:]
    return parse_emul(p.stdout, cases)


def check_against_python(results, cases, what):
    """info record, offsets, indices and bytes of every case against the rule"""
    assert len(results) == len(cases)
    for (raw_info, off, ind, data), c in zip(results, cases):
        w_info, w_off, w_ind, w_data = expected_case(c)
        tag = "%s: %s (n %d, flags %d, room %d/%d)" % (what, c.name, len(c.res), c.flags, c.max_selected, c.capacity)
        assert info_dict(raw_info) == w_info, tag
        assert np.array_equal(off, w_off), tag
        assert ind is None or np.array_equal(ind, w_ind), tag
        assert data == w_data, tag


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
_PATTERN = bytes(b for b in range(1, 256) if b != 0x0a)


def fill(n, salt=0):
    """n bytes without a 0x0a, another stretch of the pattern for another salt"""
    return (_PATTERN * (n // len(_PATTERN) + 2))[salt % len(_PATTERN):salt % len(_PATTERN) + n]


def degenerate_cases():
    out = []
    some = [fill(5, 1), b"", fill(17, 2), fill(1, 3), fill(16, 4), b"", fill(33, 5), fill(2, 6)] * 5
    for flags in ALL_FLAGS:
        out += [case("n0", [], [], flags), case("n1_kept", [fill(9)], [1], flags), case("n1_not", [fill(9)], [0], flags),
                case("n1_empty", [b""], [1], flags),
                case("all_one", some, [1] * 40, flags), case("all_zero", some, [0] * 40, flags), case("alternating", some, [0, 1] * 20, flags),
                case("first_only", some, [1] + [0] * 39, flags), case("last_only", some, [0] * 39 + [1], flags),
                case("unanswered", some, [1, 2, 0, 0xff, 1, 0, 2, 2, 0, 1] * 4, flags),
                case("only_unanswered", some, [2, 0xff] * 20, flags)]
    return out


def length_cases(T):
    """lengths around a 16-byte line and a tile, one string of more than two tiles, runs of empty strings over a tile border"""
    out = []
    lens = [0, 1, 15, 16, 17, T - 1, 0, T, T + 1, 1, 2 * T + 700, 0, 0, 3]
    strings = [fill(n, k) for k, n in enumerate(lens)]
    for flags in ALL_FLAGS:
        out.append(case("lengths", strings, [1, 0, 1, 1, 0, 1, 1, 1, 0, 1, 1, 1, 0, 1], flags, off0=3, dst_shift=5))
        for n in (T - 1, T, T + 1):
            out.append(case("one_%d" % n, [fill(n)], [0 if flags & INVERT else 1], flags))
            out.append(case("two_%d" % n, [fill(n - 1), fill(30, 9)], [0, 0] if flags & INVERT else [1, 1], flags, dst_shift=9))
        keep = 0 if flags & INVERT else 1
        # empty strings over the border of the first tile: equal offsets without NEWLINE, a run of newlines with it
        out.append(case("empties_over_border", [fill(T - 20)] + [b""] * 50 + [fill(40, 3)] + [b""] * 7, [keep] * 59, flags))
        out.append(case("empties_some_kept", [fill(T - 20)] + [b""] * 50 + [fill(40, 3)], [keep] + [keep, 1 - keep] * 25 + [keep], flags, dst_shift=1))
    # with NEWLINE a tile of nothing but one-byte strings: 16384 of them and more
    n = T + 300
    off = np.zeros(n + 1, dtype=np.uint64)
    out.append(case_of("tile_of_newlines", b"", off, np.ones(n, dtype=np.uint8), NEWLINE))
    out.append(case_of("tile_of_empties", b"", off, np.ones(n, dtype=np.uint8), 0))
    one = np.arange(n + 1, dtype=np.uint64)
    out.append(case_of("tile_of_bytes", fill(n), one, np.ones(n, dtype=np.uint8), 0, dst_shift=7))
    out.append(case_of("tile_of_bytes_nl", fill(n), one, (np.arange(n) % 3 != 0).astype(np.uint8), NEWLINE, src_shift=2))
    return out


def alignment_cases():
    """every pair (source start mod 16, destination start mod 16): offsets[0], a leading kept string's length and the shift of d_out_bytes
    vary; d_bytes itself off its line in half of them"""
    out = []
    for a in range(16):
        for d in range(16):
            lead = (a * 5 + d * 3) % 16
            strings = [fill(lead, a), fill(100, d), fill(3, a + d), b"", fill(40, 2 * a), fill(16, d)]
            flags = ALL_FLAGS[(a + d) % 4]
            keep = 0 if flags & INVERT else 1
            out.append(case("align_%d_%d" % (a, d), strings, [keep, keep, 1 - keep, keep, keep, keep], flags, off0=(a - (5 if d % 2 else 0)) % 16 + 16 * (a % 3),
                            src_shift=5 if d % 2 else 0, dst_shift=d, with_indices=(a ^ d) & 1))
    return out


def small_strings(rng, n):
    """n strings of 0 to 3 bytes as (data, off)"""
    lens = rng.integers(0, 4, size=n)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens, dtype=np.uint64)
    return fill(int(off[-1]), 11), off


def block_cases(B, scan_round):
    """string counts at the borders of the count block, and one beyond a single round of the scan workgroup"""
    rng = np.random.default_rng(20261021)
    out = []
    for n in (B - 1, B, B + 1, 3 * B + 5):
        data, off = small_strings(rng, n)
        for flags in ALL_FLAGS:
            out.append(case_of("blocks_%d" % n, data, off + np.uint64(flags), rng.integers(0, 2, size=n).astype(np.uint8), flags, dst_shift=3 * flags))
        out.append(case_of("blocks_%d_all" % n, data, off, np.ones(n, dtype=np.uint8), NEWLINE))
        out.append(case_of("blocks_%d_last_block_only" % n, data, off, (np.arange(n) >= (n - 1) // B * B).astype(np.uint8), 0))
    n = scan_round + B + 77
    lens = rng.integers(0, 2, size=n)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens, dtype=np.uint64)
    res = rng.integers(0, 2, size=n).astype(np.uint8)
    res[rng.integers(0, n, size=50)] = 2
    out.append(case_of("beyond_one_scan_round", fill(int(off[-1]), 5), off, res, NEWLINE, dst_shift=6))
    return out


def clipped(c):
    """the case with max_selected and bytes_capacity each at 0, at one short of the need and at exactly the need"""
    info, _, _, _ = expected(c.data, c.off, c.res, c.flags, len(c.res), 1 << 60)
    n_sel, n_bytes = info["n_selected"], info["n_bytes"]
    out = []
    for ms in (0, max(n_sel, 1) - 1, n_sel):
        for cap in (0, max(n_bytes, 1) - 1, n_bytes):
            out.append(c._replace(name="%s_clip_%d_%d" % (c.name, ms, cap), max_selected=ms, capacity=cap))
    return out


def clipping_cases(T):
    base = [c for c in degenerate_cases() if c.name in ("alternating", "unanswered", "n1_kept", "n0")]
    base += [c for c in length_cases(T) if c.name in ("lengths", "empties_over_border")]
    base += random_cases(T, count=6, seed=7)
    out = []
    for c in base:
        out += clipped(c)
    return out


def random_cases(T, count=200, seed=20261021):
    """`count` seeded batches of 0 to 5 output tiles: random lengths (a third of the batches short strings, a third long ones, a third
    mixed with runs of empty ones), random results (now and then a 2 or a 0xff), random flags, shifts and offsets[0]"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        target = int(rng.integers(0, 5 * T + 1))
        kind = k % 3
        lens = []
        total = 0
        while total < target:
            if kind == 0:
                n = int(rng.integers(0, 20))
            elif kind == 1:
                n = int(rng.integers(0, 3000))
            else:
                n = 0 if rng.random() < 0.6 else int(rng.integers(0, 9000 if rng.random() < 0.1 else 40))
            lens.append(n)
            total += n + 1
        n = len(lens)
        off = np.zeros(n + 1, dtype=np.uint64)
        off[1:] = np.cumsum(lens, dtype=np.uint64)
        p_keep = (0.5, 0.9, 0.1, 1.0)[int(rng.integers(0, 4))]
        res = (rng.random(n) < p_keep).astype(np.uint8)
        if n and k % 4 == 1:
            res[rng.integers(0, n, size=3)] = (2, 0xff, 2)
        data = rng.integers(0, 256, size=int(off[-1]), dtype=np.uint8).tobytes()
        out.append(case_of("random_%d" % k, data, off + np.uint64(int(rng.integers(0, 40))), res, int(rng.integers(0, 4)), int(rng.integers(0, 16)),
                           int(rng.integers(0, 16)), int(rng.integers(0, 2))))
    return out


def all_cases():
    """every case of the list, in a fixed order; the harness and the device run the same ones"""
    B, T, scan_round = geometry()
    return degenerate_cases() + length_cases(T) + alignment_cases() + block_cases(B, scan_round) + clipping_cases(T) + random_cases(T)
