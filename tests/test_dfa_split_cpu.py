"""The split path for long strings of memory-less automata, the part that can be wrong without a GPU (csrc/dfa_split_core.h: chunk
geometry, the adaptive chunk size, the map of a chunk, the composition of maps), compiled for the host (tests/emul/dfa_split_emul.cpp)
and run against the CPU restatement.  The kernels around it are checked by tests/test_dfa_split_gpu.py."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import oracle_lib
from mfa_amd import image

EMUL_DIR = os.path.join(oracle_lib.ROOT, "tests", "emul")

with open(os.path.join(oracle_lib.GOLDEN, "manifest.json")) as f:
    NFA_NAMES = [a["name"] for a in json.load(f)["automata"] if a["name"].startswith("nfa_")]


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dfa_split_emul") / "dfa_split_emul")
    subprocess.check_call([os.path.join(EMUL_DIR, "build_dfa_split.sh"), exe], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return exe


def blob_of(name, rev):
    img = image.parse_dump(oracle_lib.load_dump(name))
    if rev:
        img["reversed"] = 1
    return image.to_blob(img)


def strings_for(name, rng):
    """strings of 0 to 20 000 bytes, packed back to back so that they start at every offset mod 16; many are accepted, many are
    rejected by their last byte only, some die early"""
    tails = {"nfa_abb": b"abb", "nfa_third": b"abb", "nfa_enum": b"abc", "nfa_star1": b"ab", "nfa_star2": b"a", "nfa_star4": b"a", "nfa_alt3": b"c" * 40}
    tail = next((v for k, v in tails.items() if name.startswith(k)), b"abb")
    alpha = b"abc" if name.startswith(("nfa_enum", "nfa_dot")) else b"ab"
    lens = [0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 100, 255, 256, 257, 4095, 4096, 4097, 8191, 12288, 20000, 19999]
    lens += [int(x) for x in rng.integers(0, 20001, size=14)] + [int(x) for x in rng.integers(0, 200, size=40)]
    out, at, k = [], 0, 0
    while lens or len({o % 16 for o in out_offsets(out)}) < 16:
        ln = lens.pop(0) if lens else int(rng.integers(1, 300))
        if name.startswith("nfa_alt3"):
            body = b"ab" + b"".join(rng.choice([b"ab", b"ba"]) for _ in range(ln // 2))
            s = (body[:max(ln - len(tail), 0)] + tail)[:ln] if ln >= 2 else body[:ln]
        elif name.startswith("nfa_star4"):
            body = b"".join(rng.choice([b"ab", b"c", b"cc", b"abab"]) for _ in range(ln // 2 + 1))[:max(ln - 1, 0)]
            while body and body[-1:] == b"a":          # cut inside a word: drop the open `a`
                body = body[:-1]
            s = body + b"a" if ln else b""
        else:
            s = bytes(rng.choice(list(alpha), size=ln).tolist())
            if ln >= len(tail) and k % 3 != 2:
                s = s[:ln - len(tail)] + tail
        if k % 4 == 1 and s:
            s = s[:-1] + b"z"                              # rejected by the last byte only
        if k % 11 == 5 and len(s) > 40:
            s = s[:7] + b"\x00" + s[8:]                    # dies in its first chunk (or not at all: `.`)
        out.append(s)
        at += len(s)
        k += 1
    return out


def out_offsets(strings):
    at, offs = 0, []
    for s in strings:
        offs.append(at)
        at += len(s)
    return offs


def expected_geometry(off, chunk_min, arena):
    long_bytes = int(off[-1])
    chunk = max(chunk_min, (long_bytes // arena + 15) // 16 * 16)
    chunks = sum((int(e) - (int(b) & ~15) + chunk - 1) // chunk for b, e in zip(off[:-1], off[1:]) if e > b)
    return chunk, chunks


@pytest.mark.parametrize("rev", [0, 1], ids=["forward", "reversed"])
@pytest.mark.parametrize("name", NFA_NAMES)
def test_split_core_against_oracle(emul, name, rev, tmp_path):
    rng = np.random.default_rng(len(name) * 131 + rev)
    blob = blob_of(name, rev)
    (tmp_path / "a.blob").write_bytes(blob)
    strings = strings_for(name, rng)
    if rev:
        strings = [s[::-1] for s in strings]               # the flag makes the same automaton scan from the end: the mirrored language
    assert {o % 16 for o in out_offsets(strings)} == set(range(16)) and max(len(s) for s in strings) == 20000 and min(len(s) for s in strings) == 0
    data, off = oracle_lib.pack(strings)
    want = oracle_lib.OracleImage(blob).match(strings)
    (tmp_path / "batch.bin").write_bytes(struct.pack("<Q", len(strings)) + off.astype("<u8").tobytes() + data.tobytes()[:int(off[-1])])
    # (chunk_min, arena chunks, bytes of maps per fold tile): the last two rows make the device's formula choose a larger chunk
    for chunk_min, arena, tile in ((16, 1 << 20, 2048), (48, 1 << 20, 1024), (4096, 1 << 20, 32768), (16, 3000, 32768), (48, 7, 512)):
        p = subprocess.run([emul, str(tmp_path / "a.blob"), str(tmp_path / "batch.bin"), str(chunk_min), str(arena), str(tile)], capture_output=True)
        assert p.returncode == 0, p.stderr.decode()[-400:]
        lines = p.stdout.split()
        assert (int(lines[0]), int(lines[1])) == expected_geometry(off, chunk_min, arena), (chunk_min, arena)
        got = np.array([int(x) for x in lines[2:]], dtype=np.uint8)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, "%s chunk_min %d arena %d: %d mismatches, first len %d at offset %d want %d" % (
            name, chunk_min, arena, bad.size, len(strings[bad[0]]), int(off[bad[0]]), want[bad[0]])
    if not rev and not name.startswith("nfa_dot"):        # the generator does its job: both answers occur (forward; nfa_dot_* die on every input)
        assert 0 < want.sum() < len(strings)
