"""The split path for long strings of memory-less automata, the part that can be wrong without a GPU (csrc/dfa_split_core.h: chunk
geometry, the adaptive chunk size, the map of a chunk, the composition of maps), compiled for the host (tests/emul/dfa_split_emul.cpp)
and run against the CPU restatement.  The kernels around it are checked by tests/test_dfa_split_gpu.py."""
import subprocess

import numpy as np
import pytest

import oracle_lib
from testlib import NFA_NAMES, blob_of, emul_exe, out_offsets, strings_for, write_batch


@pytest.fixture(scope="module")
def emul():
    return emul_exe("dfa_split")


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
    want = oracle_lib.OracleImage(blob).match(strings)
    _, off = write_batch(tmp_path / "batch.bin", strings)
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
