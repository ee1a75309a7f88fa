"""What tests/test_nfa_set_resume_cpu.py and tests/test_nfa_set_resume_gpu.py share: the host harness tests/emul/nfa_set_resume_emul.cpp
built once per session, its input files and its output, and the records of mfa_match_batch_resume_set on the device -- TEST
INFRASTRUCTURE ONLY: no tests, no fixtures, no marks in here.  torch is imported where it is used, so that collecting the CPU tests needs
no GPU."""
import atexit
import os
import shutil
import struct
import subprocess
import tempfile

import numpy as np

import oracle_lib
from mfa_amd import capi, image
from testlib import EMUL_DIR, cuts_for, filled, rounds_of, upload, write_batch

WORDS = capi.SET_STATE_WORDS
START, LIVE, INVALID = capi.SET_STATE_START, capi.SET_STATE_LIVE, capi.SET_STATE_INVALID
CSRC = os.path.join(oracle_lib.ROOT, "re2-modification_amd", "csrc")

_built = {}


def resume_emul_exe(flags=""):
    """tests/emul/nfa_set_resume_emul.cpp, built with the g++ line tests/emul/build.sh has for its nfa_set row (that script has no row for
    this name) and `flags` behind the caller's EMUL_FLAGS, once per session, in a temporary directory of its own; the compiler is heard
    only when it fails"""
    if flags not in _built:
        folder = tempfile.mkdtemp(prefix="nfa_set_resume_emul_")
        atexit.register(shutil.rmtree, folder, ignore_errors=True)
        exe = os.path.join(folder, "nfa_set_resume_emul")
        cmd = (["g++", "-O1", "-g", "-std=c++17"] + (os.environ.get("EMUL_FLAGS", "") + " " + flags).split()
               + ["-Wall", "-Ishim", "-Wno-unknown-pragmas", "-Wno-unused-function", "-Wno-unused-variable", "-I" + CSRC,
                  "-I" + os.path.join(oracle_lib.ROOT, "include"), "-o", exe, "nfa_set_resume_emul.cpp", os.path.join(CSRC, "image_host.cpp")])
        p = subprocess.run(cmd, cwd=EMUL_DIR, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert p.returncode == 0, "building nfa_set_resume_emul failed:\n%s" % p.stdout
        _built[flags] = exe
    return _built[flags]


def mask_words(n_nodes):
    return 1 if n_nodes <= 32 else 2 if n_nodes <= 64 else 4 if n_nodes <= 128 else 8


def record(tag, nodes=(), reserved=(0, 0, 0)):
    """one record as twelve words: tag, reserved[3], nodes[8] (node v: bit v & 31 of nodes[v >> 5]); nodes: the words, from the first"""
    nodes = list(nodes) + [0] * (8 - len(nodes))
    return np.array([tag] + list(reserved) + nodes, dtype=np.uint32)


def run_pieces(exe, tmp_path, blob, strings, rounds, states=None):
    """the harness's `pieces` mode: rounds[r][k] = (begin, end) of string k's piece in round r, relative to the string.  Returns (one
    array of result digits per round, the final records as an [n, WORDS] array of uint32)"""
    (tmp_path / "a.blob").write_bytes(blob)
    write_batch(tmp_path / "batch.bin", strings)
    flat = np.array([[p for p in row] for row in rounds], dtype="<u8").reshape(-1)
    (tmp_path / "cuts.bin").write_bytes(struct.pack("<Q", len(rounds)) + flat.tobytes())
    cmd = [exe, "pieces", str(tmp_path / "a.blob"), str(tmp_path / "batch.bin"), str(tmp_path / "cuts.bin")]
    if states is not None:
        (tmp_path / "states.bin").write_bytes(np.ascontiguousarray(states, dtype="<u4").tobytes())
        cmd.append(str(tmp_path / "states.bin"))
    p = subprocess.run(cmd, capture_output=True)
    assert p.returncode == 0, p.stderr.decode()[-600:]
    lines = p.stdout.decode().split("\n")
    n = len(strings)
    digits = [np.frombuffer(ln.encode(), dtype=np.uint8) - ord("0") for ln in lines[:len(rounds)]]
    assert all(len(d) == n for d in digits)
    recs = np.array([[int(w, 16) for w in ln.split()] for ln in lines[len(rounds):len(rounds) + n]], dtype=np.uint32).reshape(n, WORDS)
    return digits, recs


def run_table(exe, tmp_path, blob, strings):
    """the harness's `table` mode; returns the words of its "ok STRINGS STATES W" line"""
    (tmp_path / "a.blob").write_bytes(blob)
    write_batch(tmp_path / "batch.bin", strings)
    p = subprocess.run([exe, "table", str(tmp_path / "a.blob"), str(tmp_path / "batch.bin")], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()[-600:]
    f = p.stdout.split()
    assert f[0] == b"ok"
    return [int(x) for x in f[1:]]


def whole(strings):
    """one round: every string whole"""
    return [[(0, len(s)) for s in strings]]


def piece_rounds(blob, strings, rng):
    """(ROUNDS rounds of cut strings in scan order as testlib.rounds_of gives them, whether the image scans from the end)"""
    is_rev = image.blob_info(blob)["reversed"]
    return rounds_of(strings, cuts_for(strings, rng), is_rev), is_rev


def check_records_are_clean(recs, n_nodes):
    """what the contract promises of every record on return: tag LIVE or INVALID, reserved zero, nothing beyond the mask width, nothing
    for a node the image lacks, an INVALID record's nodes zero"""
    W = mask_words(n_nodes)
    assert set(np.unique(recs[:, 0])) <= {LIVE, INVALID}
    assert not recs[:, 1:4].any() and not recs[:, 4 + W:].any()
    have = np.zeros(8, dtype=np.uint32)
    for v in range(n_nodes):
        have[v >> 5] |= np.uint32(1 << (v & 31))
    assert not (recs[:, 4:] & ~have).any()
    assert not recs[recs[:, 0] == INVALID, 4:].any()


# ---- on the device ------------------------------------------------------------------------------------------------------------------------
def new_records(n, rows=None):
    """n zeroed records on the device (every string at its start), or the given [n, WORDS] array"""
    import torch
    host = np.zeros((max(n, 1), WORDS), dtype=np.uint32) if rows is None else np.ascontiguousarray(rows, dtype=np.uint32)
    return torch.from_numpy(host.view(np.int32).reshape(-1).copy()).cuda()


def records_of(d_states, n):
    return d_states.cpu().numpy().view(np.uint32)[:n * WORDS].reshape(n, WORDS).copy()


def feed_set(img, pieces, d_states, results=True, stream=None):
    """one round: the pieces of all strings through mfa_match_batch_resume_set, the batch in exactly the room the read rule asks for;
    returns the result bytes (None without results)"""
    import torch
    d_bytes, d_off, _ = upload(pieces, exact=True)
    res = filled(len(pieces)) if results else None
    img.match_tensors_resume_set(d_bytes, d_off, d_states, res, stream=stream)
    torch.cuda.synchronize()
    return res[:len(pieces)].cpu().numpy() if results else None
