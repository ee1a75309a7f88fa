"""What tests/test_nfa_set_wave_resume_cpu.py and tests/test_nfa_set_wave_resume_gpu.py share: the host harness
tests/emul/nfa_set_wave_resume_emul.cpp built once per session, its input files and its output, the cuts both feed, and the wide records
of mfa_match_batch_resume_set_wide on the device -- TEST INFRASTRUCTURE ONLY: no tests, no fixtures, no marks in here.  torch is imported
where it is used, so that collecting the CPU tests needs no GPU."""
import atexit
import os
import shutil
import struct
import subprocess
import tempfile

import numpy as np

import oracle_lib
from mfa_amd import capi, image
from setwave_lib import CSRC, words_of
from testlib import EMUL_DIR, MAX_BYTES, ROUNDS, cuts_for, rounds_of, upload

WORDS = capi.SET_STATE_WIDE_WORDS
START, LIVE, INVALID = capi.SET_STATE_START, capi.SET_STATE_LIVE, capi.SET_STATE_INVALID
N_ROUNDS = 3
GUARD = 0x5a5a5a5a
FIXED_LENGTHS = (0, 1, 15, 16, 17, 1023, 1024, 1025)

_built = {}


def resume_emul_exe(flags=""):
    """tests/emul/nfa_set_wave_resume_emul.cpp, built with the g++ line of setwave_lib.wave_emul_exe (-O2: the harness does 64 lanes'
    work per step) and `flags` behind the caller's EMUL_FLAGS, once per session, in a temporary directory of its own; the compiler is
    heard only when it fails"""
    if flags not in _built:
        folder = tempfile.mkdtemp(prefix="nfa_set_wave_resume_emul_")
        atexit.register(shutil.rmtree, folder, ignore_errors=True)
        exe = os.path.join(folder, "nfa_set_wave_resume_emul")
        cmd = (["g++", "-O2", "-g", "-std=c++17"] + (os.environ.get("EMUL_FLAGS", "") + " " + flags).split()
               + ["-Wall", "-Ishim", "-Wno-unknown-pragmas", "-Wno-unused-function", "-Wno-unused-variable", "-I" + CSRC,
                  "-I" + os.path.join(oracle_lib.ROOT, "include"), "-o", exe, "nfa_set_wave_resume_emul.cpp", os.path.join(CSRC, "image_host.cpp")])
        p = subprocess.run(cmd, cwd=EMUL_DIR, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert p.returncode == 0, "building nfa_set_wave_resume_emul failed:\n%s" % p.stdout
        _built[flags] = exe
    return _built[flags]


def record(tag, nodes=(), reserved=(0, 0, 0)):
    """one record as 68 words: tag, reserved[3], nodes[64] (node v: bit v & 31 of nodes[v >> 5]); nodes: the words from the first, or a
    dict word -> value"""
    row = np.zeros(WORDS, dtype=np.uint32)
    row[0] = tag
    row[1:4] = reserved
    for k, w in (nodes.items() if isinstance(nodes, dict) else enumerate(nodes)):
        row[4 + k] = w
    return row


# ---- the harness ----------------------------------------------------------------------------------------------------------------------
def raw_round(offsets, data):
    """a round given by its offsets alone (they may point outside `data`)"""
    return ("raw", [int(x) for x in offsets], bytes(data))


def _round_file(path, rnd):
    if isinstance(rnd, tuple) and rnd[0] == "raw":
        off, data = rnd[1], rnd[2]
    else:
        off, data = [0] + [int(x) for x in np.cumsum([len(p) for p in rnd])], b"".join(rnd)
    path.write_bytes(struct.pack("<QQ", len(off) - 1, len(data)) + np.asarray(off, dtype="<u8").tobytes() + data)
    return len(off) - 1


def run_pieces(exe, tmp_path, blob, rounds, states=None):
    """the harness's `pieces` mode: rounds[r] is the list of the strings' pieces of round r, as one call gets them, or a raw_round.
    Returns ((table words, W, depth), one array of result digits per round, the final records as an [n, WORDS] array of uint32)"""
    (tmp_path / "a.blob").write_bytes(blob)
    cmd = [exe, "pieces", str(tmp_path / "a.blob"), "-"]
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
    head = lines[0].split()
    assert head[0] == "tables"
    digits = [np.frombuffer(ln.encode(), dtype=np.uint8) - ord("0") for ln in lines[1:1 + len(rounds)]]
    assert all(len(d) == n for d in digits)
    recs = np.array([[int(w, 16) for w in ln.split()] for ln in lines[1 + len(rounds):1 + len(rounds) + n]], dtype=np.uint32).reshape(n, WORDS)
    return tuple(int(x) for x in head[1:]), digits, recs


def run_table(exe, tmp_path, blob, strings):
    """the harness's `table` mode: ((table words, W, depth), strings, states)"""
    from testlib import write_batch
    (tmp_path / "a.blob").write_bytes(blob)
    write_batch(tmp_path / "batch.bin", strings)
    p = subprocess.run([exe, "table", str(tmp_path / "a.blob"), str(tmp_path / "batch.bin")], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()[-1200:]
    head, ok = [ln.split() for ln in p.stdout.decode().split("\n")[:2]]
    assert head[0] == "tables" and ok[0] == "ok"
    return tuple(int(x) for x in head[1:]), int(ok[1]), int(ok[2])


def tables_in_lds(tables):
    """whether the four stacks and the tables fit the 64 KiB a block may take, from the harness's "tables WORDS W DEPTH" line"""
    words, _, depth = tables
    return (4 * depth + words) * 4 <= 65536


# ---- cuts -------------------------------------------------------------------------------------------------------------------------------
def three_rounds(blob, strings, rng):
    """(N_ROUNDS lists of (begin, end) per string, relative to the string, in scan order; whether the image scans from the end): the cuts
    of testlib.cuts_for and rounds_of with the pieces of their last two rounds, which lie side by side, fed as one"""
    is_rev = image.blob_info(blob)["reversed"]
    four = rounds_of(strings, cuts_for(strings, rng), is_rev)
    assert ROUNDS == N_ROUNDS + 1
    last = [(min(a[0], b[0]), max(a[1], b[1])) for a, b in zip(four[2], four[3])]
    assert all(a[1] == b[0] or b[1] == a[0] or a[0] == a[1] or b[0] == b[1] for a, b in zip(four[2], four[3]))
    return [four[0], four[1], last], is_rev


def fixed_cuts(pick, is_rev):
    """strings made for cuts the kernel can get wrong: (strings, rounds as three_rounds gives them).  Pieces of every length of
    FIXED_LENGTHS in every round, empty pieces in the middle round between pieces that are not, and fillers until in EVERY round's
    buffer, where the pieces lie back to back, a piece that is not empty starts at every offset mod 16.  pick(ln): ln bytes of text"""
    L = FIXED_LENGTHS
    triples = [(L[(k + 1) % 8], L[(3 * k) % 8], L[(k + 3) % 8]) for k in range(8)] + [(a, 0, b) for a, b in ((1, 15), (16, 17), (1023, 1), (1024, 1025), (17, 1024))]
    triples += [(0, 0, 0), (0, 5, 0), (1025, 1025, 1025), (1024, 1024, 1024)]

    def starts(r):
        at, seen = 0, set()
        for t in triples:
            if t[r]:
                seen.add(at % 16)
            at += t[r]
        return seen

    k = 0
    while any(len(starts(r)) < 16 for r in range(N_ROUNDS)):
        triples.append((1 + k % 7, 1 + k % 5, 1 + k % 3))
        k += 1
        assert k < 400
    for r in range(N_ROUNDS):
        assert set(L) <= {t[r] for t in triples}
    strings = [pick(sum(t)) for t in triples]
    rounds = [[], [], []]
    for s, (a, b, c) in zip(strings, triples):
        n = len(s)
        cuts = [(n - a, n), (n - a - b, n - a), (0, n - a - b)] if is_rev else [(0, a), (a, a + b), (a + b, n)]
        for r in range(N_ROUNDS):
            rounds[r].append(cuts[r])
    return strings, rounds


def pieces_of(strings, row):
    return [s[b:e] for s, (b, e) in zip(strings, row)]


def whole(strings):
    return [[(0, len(s)) for s in strings]]


def check_records_are_clean(recs, n_nodes):
    """what the contract promises of every record on return: tag LIVE or INVALID, reserved zero, nothing at or beyond W, nothing for a
    node the image lacks, an INVALID record's nodes zero"""
    W = words_of(n_nodes)
    assert set(np.unique(recs[:, 0])) <= {LIVE, INVALID}
    assert not recs[:, 1:4].any() and not recs[:, 4 + W:].any()
    have = np.zeros(64, dtype=np.uint32)
    for v in range(n_nodes):
        have[v >> 5] |= np.uint32(1 << (v & 31))
    assert not (recs[:, 4:] & ~have).any()
    assert not recs[recs[:, 0] == INVALID, 4:].any()


# ---- the record's checks (the 303-node counter) ---------------------------------------------------------------------------------------
def sticky_case():
    """the records and the two rounds of the sticky-error test, for the 303-node counter (which scans forward), shared with the GPU test:
    (rows, rounds as raw_round, the strings the good records have been given after each round, indices of the errors, index of the
    dead record, indices of the good records)"""
    piece = b"a" * 150
    rows = [record(2), record(START), record(INVALID), record(LIVE, [1], (0, 5, 0)), record(START, [], (1, 0, 0)), record(START, [0xdeadbeef] * 64),
            record(LIVE, {9: 1 << 15}), record(LIVE, {0: 1, 10: 1}), record(START), record(LIVE, {0: 1, 63: 1 << 31}), record(LIVE), record(START)]
    errors, dead, good, too_long = [0, 2, 3, 4, 6, 7, 9, 11], 10, [1, 5, 8], 11
    n = len(rows)
    # round 1: 150 bytes each; the dead record's and the over-long record's offsets point outside the buffer: their bytes are not read
    body = piece * (n - 2)
    off1 = [150 * k for k in range(n - 1)] + [len(body) + 4096, len(body) + 4096 + MAX_BYTES + 1]
    assert off1[dead + 1] - off1[dead] == 4096 and off1[too_long + 1] - off1[too_long] == MAX_BYTES + 1 and off1[dead] == len(body)
    off2 = [150 * k for k in range(n + 1)]
    return np.stack(rows), [raw_round(off1, body), raw_round(off2, piece * n)], [[piece] * 3, [piece * 2] * 3], errors, dead, good


def check_sticky(blob, digits, recs_by_round, what):
    rows, _, given, errors, dead, good = sticky_case()
    ora = oracle_lib.OracleImage(blob)
    for r in range(2):
        want = np.zeros(len(rows), dtype=np.uint8)
        want[errors] = 2
        want[good] = ora.match(given[r])
        assert list(digits[r]) == list(want), "%s round %d" % (what, r)
        recs = recs_by_round[r]
        assert (recs[errors, 0] == INVALID).all() and not recs[errors, 1:].any(), what
        assert list(recs[dead]) == [LIVE] + [0] * (WORDS - 1), what
        assert (recs[good, 0] == LIVE).all() and recs[good, 4:].any(axis=1).all() and np.array_equal(recs[good[0]], recs[good[1]]) and np.array_equal(recs[good[0]], recs[good[2]]), what
        check_records_are_clean(recs, 303)
    assert list(ora.match(given[1])) == [1, 1, 1] and list(ora.match(given[0])) == [0, 0, 0]


# ---- on the device ------------------------------------------------------------------------------------------------------------------------
def new_records(n, rows=None):
    """n zeroed records on the device (every string at its start), or the given [n, WORDS] array, with a guard quarter of 16 bytes in
    front and behind: the whole buffer; the records are records_view(buf, n)"""
    import torch
    host = np.full((max(n, 1) * WORDS + 8,), GUARD, dtype=np.uint32)
    host[4:4 + max(n, 1) * WORDS] = 0 if rows is None else np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1)
    return torch.from_numpy(host.view(np.int32).copy()).cuda()


def records_view(buf, n):
    view = buf[4:4 + max(n, 1) * WORDS]
    assert view.data_ptr() % 16 == 0
    return view


def records_of(buf, n):
    """the records, after a look at the guard quarters"""
    host = buf.cpu().numpy().view(np.uint32)
    assert (host[:4] == GUARD).all() and (host[4 + max(n, 1) * WORDS:] == GUARD).all(), "a record word outside the records"
    return host[4:4 + n * WORDS].reshape(n, WORDS).copy()


def call_wide(img, d_bytes, d_off, buf, n, results=True, stream=None):
    """one mfa_match_batch_resume_set_wide call on uploaded pieces, NOT synchronised: the guarded result buffer (64 bytes of 7 on either
    side), or None"""
    import torch
    res = torch.full((n + 128,), 7, dtype=torch.uint8, device="cuda") if results else None
    img.match_tensors_resume_set_wide(d_bytes, d_off, records_view(buf, n), res[64:64 + n] if results else None, stream=stream)
    return res


def results_of(res, n):
    host = res.cpu().numpy()
    assert (host[:64] == 7).all() and (host[64 + n:] == 7).all(), "a result byte outside the results"
    return host[64:64 + n].copy()


def feed_wide(img, pieces, buf, results=True, stream=None):
    """one round: the pieces of all strings through mfa_match_batch_resume_set_wide, the batch in exactly the room the read rule asks
    for; returns the result bytes (None without results)"""
    import torch
    d_bytes, d_off, _ = upload(pieces, exact=True)
    res = call_wide(img, d_bytes, d_off, buf, len(pieces), results, stream)
    torch.cuda.synchronize()
    return results_of(res, len(pieces)) if results else None
