"""What tests/test_nfa_set_wave_split_cpu.py and tests/test_nfa_set_wave_split_gpu.py share: the host harness
tests/emul/nfa_set_wave_split_emul.cpp built once per session, its input files and its output -- TEST INFRASTRUCTURE ONLY: no tests, no
fixtures, no marks in here."""
import atexit
import os
import shutil
import subprocess
import tempfile

import numpy as np

import oracle_lib
from setwave_lib import CSRC
from setwaveresume_lib import WORDS, _round_file
from testlib import EMUL_DIR, write_batch

# a literal prefix in front of a loop of more than 256 nodes: a walk from {start} dies in mid-text
PREFIX_WIDE = "xyz(a|b)*a" + "(a|b)" * 52

_built = {}


def wave_split_emul_exe(flags=""):
    """tests/emul/nfa_set_wave_split_emul.cpp, built with the g++ line of setsplit_lib.split_emul_exe (-O2: the harness does 64 lanes'
    work per step and walks every string several times) and `flags` behind the caller's EMUL_FLAGS, once per session, in a temporary
    directory of its own; the compiler is heard only when it fails"""
    if flags not in _built:
        folder = tempfile.mkdtemp(prefix="nfa_set_wave_split_emul_")
        atexit.register(shutil.rmtree, folder, ignore_errors=True)
        exe = os.path.join(folder, "nfa_set_wave_split_emul")
        cmd = (["g++", "-O2", "-g", "-std=c++17"] + (os.environ.get("EMUL_FLAGS", "") + " " + flags).split()
               + ["-Wall", "-Ishim", "-Wno-unknown-pragmas", "-Wno-unused-function", "-Wno-unused-variable", "-I" + CSRC,
                  "-I" + os.path.join(oracle_lib.ROOT, "include"), "-o", exe, "nfa_set_wave_split_emul.cpp", os.path.join(CSRC, "image_host.cpp")])
        p = subprocess.run(cmd, cwd=EMUL_DIR, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert p.returncode == 0, "building nfa_set_wave_split_emul failed:\n%s" % p.stdout
        _built[flags] = exe
    return _built[flags]


KEYS = ("W", "checks", "rewalked", "serial_strings", "serial_bytes", "home_nodes", "home_guesses", "invalid_ends")
COUNT_KEYS = ("rewalked", "serial_strings", "serial_bytes")


def run_wave_split(exe, tmp_path, blob, strings, chunks, lookbacks, rounds, depth=None, run=None):
    """the harness's `split` mode on every combination of the three lists, chunks outermost: a list of ((chunk, lookback, rounds), counts,
    result digits).  depth: the stacks' slots, instead of the tables' own.  run: what runs the command line instead of subprocess.run --
    it returns the finished process, or None for "refused", which is returned as it is"""
    (tmp_path / "a.blob").write_bytes(blob)
    write_batch(tmp_path / "batch.bin", strings)
    as_list = lambda v: ",".join(str(x) for x in v)
    cmd = [exe, "split", str(tmp_path / "a.blob"), str(tmp_path / "batch.bin"), as_list(chunks), as_list(lookbacks), as_list(rounds)]
    cmd += [str(depth)] if depth is not None else []
    p = subprocess.run(cmd, capture_output=True) if run is None else run(cmd)
    if p is None:
        return None
    assert p.returncode == 0, p.stderr.decode()[-600:]
    lines = p.stdout.split(b"\n")
    combos = [(c, lb, r) for c in chunks for lb in lookbacks for r in rounds]
    out = []
    for i, combo in enumerate(combos):
        w = lines[2 * i].split()
        assert w[0] == b"ok" and len(w) == 1 + len(KEYS), lines[2 * i]
        out.append((combo, dict(zip(KEYS, (int(x) for x in w[1:]))), np.frombuffer(lines[2 * i + 1], dtype=np.uint8) - ord("0")))
    return out


def run_wave_split_pieces(exe, tmp_path, blob, rounds, chunk, lookback, repair_rounds, split_min, states=None):
    """the harness's `pieces` mode: rounds[r] is the list of the strings' pieces of round r, or a setwaveresume_lib.raw_round.  Returns
    (one array of result digits per round, the count of queued pieces per round, the final records as an [n, WORDS] array of uint32)"""
    (tmp_path / "a.blob").write_bytes(blob)
    cmd = [exe, "pieces", str(tmp_path / "a.blob"), "-", str(chunk), str(lookback), str(repair_rounds), str(split_min)]
    if states is not None:
        (tmp_path / "states.bin").write_bytes(np.ascontiguousarray(states, dtype="<u4").tobytes())
        cmd[3] = str(tmp_path / "states.bin")
    n = None
    for r, rnd in enumerate(rounds):
        n_here = _round_file(tmp_path / ("round%d.bin" % r), rnd)
        assert n in (None, n_here)
        n = n_here
        cmd.append(str(tmp_path / ("round%d.bin" % r)))
    p = subprocess.run(cmd, capture_output=True)
    assert p.returncode == 0, p.stderr.decode()[-1200:]
    lines = p.stdout.decode().split("\n")
    assert lines[0].split()[0] == "tables"
    digits, queued = [], []
    for ln in lines[1:1 + len(rounds)]:
        f = ln.split()                                                    # (no string: the digits are empty)
        digits.append(np.frombuffer(f[0].encode() if len(f) == 2 else b"", dtype=np.uint8) - ord("0"))
        queued.append(int(f[-1]))
    assert all(len(d) == n for d in digits)
    recs = np.array([[int(w, 16) for w in ln.split()] for ln in lines[1 + len(rounds):1 + len(rounds) + n]], dtype=np.uint32).reshape(n, WORDS)
    return digits, queued, recs
