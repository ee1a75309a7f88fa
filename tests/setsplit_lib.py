"""What tests/test_nfa_set_split_cpu.py and tests/test_nfa_set_split_gpu.py share: the host harness tests/emul/nfa_set_split_emul.cpp built
once per session, its input files and its output, and the corpora both walk -- TEST INFRASTRUCTURE ONLY: no tests, no fixtures, no marks
in here."""
import atexit
import os
import shutil
import subprocess
import tempfile

import numpy as np

import oracle_lib
from mfa_amd import image
from testlib import EMUL_DIR, accepted_of, blob_of, front_end_blob, k_regex, out_offsets, write_batch

CSRC = os.path.join(oracle_lib.ROOT, "re2-modification_amd", "csrc")
CHUNKS = (16, 32, 64)
LOOKBACKS = (0, 8, 256)
ROUNDS = (0, 1, 3, 8)
# (a^300)* has 303 nodes, more than a set-walk image holds (256): the counter here is the longest round one that fits, 253 nodes, W = 8
COUNTER = "(" + "a" * 250 + ")*"
PREFIX = "xyz(a|b)*abb"                 # a literal prefix in front of a loop: a walk from {start} dies in mid-text

_built = {}


def split_emul_exe(flags=""):
    """tests/emul/nfa_set_split_emul.cpp, built with a g++ line of its own (the one tests/setresume_lib.py has, at -O2: this harness walks
    every string several times) and `flags` behind the caller's EMUL_FLAGS, once per session, in a temporary directory of its own; the
    compiler is heard only when it fails"""
    if flags not in _built:
        folder = tempfile.mkdtemp(prefix="nfa_set_split_emul_")
        atexit.register(shutil.rmtree, folder, ignore_errors=True)
        exe = os.path.join(folder, "nfa_set_split_emul")
        cmd = (["g++", "-O2", "-g", "-std=c++17"] + (os.environ.get("EMUL_FLAGS", "") + " " + flags).split()
               + ["-Wall", "-Ishim", "-Wno-unknown-pragmas", "-Wno-unused-function", "-Wno-unused-variable", "-I" + CSRC,
                  "-I" + os.path.join(oracle_lib.ROOT, "include"), "-o", exe, "nfa_set_split_emul.cpp", os.path.join(CSRC, "image_host.cpp")])
        p = subprocess.run(cmd, cwd=EMUL_DIR, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert p.returncode == 0, "building nfa_set_split_emul failed:\n%s" % p.stdout
        _built[flags] = exe
    return _built[flags]


KEYS = ("W", "checks", "rewalked", "serial_strings", "serial_bytes", "home_nodes", "home_guesses")


def run_split(exe, tmp_path, blob, strings, chunks, lookbacks, rounds, mode="one", run=None):
    """the harness on every combination of the three lists, chunks outermost: a list of ((chunk, lookback, rounds), counts, result digits).
    run: what runs the command line instead of subprocess.run -- it returns the finished process, or None for "refused", which is
    returned as it is"""
    (tmp_path / "a.blob").write_bytes(blob)
    write_batch(tmp_path / "batch.bin", strings)
    as_list = lambda v: ",".join(str(x) for x in v)
    cmd = [exe, str(tmp_path / "a.blob"), str(tmp_path / "batch.bin"), as_list(chunks), as_list(lookbacks), as_list(rounds), mode]
    p = subprocess.run(cmd, capture_output=True) if run is None else run(cmd)
    if p is None:
        return None
    assert p.returncode == 0, p.stderr.decode()[-600:]
    lines = p.stdout.split(b"\n")
    combos = [(c, lb, r) for c in chunks for lb in lookbacks for r in rounds]
    out = []
    for i, combo in enumerate(combos):
        w = lines[2 * i].split()
        assert w[0] == b"ok", lines[2 * i]
        out.append((combo, dict(zip(KEYS, (int(x) for x in w[1:]))), np.frombuffer(lines[2 * i + 1], dtype=np.uint8) - ord("0")))
    return out


def chunk_lengths():
    """lengths around multiples of every chunk size, +-1, and the ends of the range"""
    lens = {0, 1, 2, 700}
    for c in CHUNKS:
        for m in (1, 2, 3, 5):
            lens |= {m * c - 1, m * c, m * c + 1}
    return sorted(lens)


def fixture_corpus(name, rev):
    """(blob, strings) for a memory-less fixture: an accepted string and one rejected by its last byte only for every length of
    chunk_lengths, some that die early; packed back to back they start at every offset mod 16.  rev: the image is made to scan from the
    end and the strings are mirrored (as testlib.setwalk_corpus does it)"""
    rng = np.random.default_rng(len(name) * 389 + rev)
    strings, k = [], 0
    lens = chunk_lengths()
    lens = lens + lens
    while lens or len({o % 16 for o in out_offsets(strings)}) < 16:
        ln = lens.pop(0) if lens else int(rng.integers(1, 40))
        s = accepted_of(name, ln, rng)[-ln:] if ln else b""
        assert len(s) == ln
        if k % 3 == 1 and s:
            s = s[:-1] + b"z"
        if k % 7 == 5 and len(s) > 40:
            s = s[:7] + b"\x00" + s[8:]
        strings.append(s)
        k += 1
    blob = blob_of(name, rev)
    if rev and not image.blob_info(blob_of(name, 0))["reversed"]:
        strings = [s[::-1] for s in strings]
    return blob, strings


def ab_strings(lens, rng, tail=b""):
    return [(np.frombuffer(b"ab", dtype=np.uint8)[rng.integers(0, 2, size=max(ln - len(tail), 0))].tobytes() + tail)[:ln] for ln in lens]


def k_blob(k, tmp_path, rev=0):
    """(a|b)*a(a|b)^k, Thompson: the set is fixed by the last k + 1 bytes"""
    return front_end_blob(k_regex(k), tmp_path, rev)
