"""What the tests of the memory-less engines share, and the tools that replay them: the fixtures' and the front-end's blobs, batches on the
device, the state words of the resume call, the corpora more than one file walks, and the host harnesses of tests/emul/ built once per
session -- TEST INFRASTRUCTURE ONLY: no tests, no fixtures, no marks in here.  torch is imported where it is used, so that collecting
the CPU tests needs no GPU."""
import atexit
import json
import os
import re
import shutil
import struct
import subprocess
import tempfile

import numpy as np

import oracle_lib
from mfa_amd import capi, image

DIPLOMA = os.path.join(oracle_lib.ROOT, "re2-modification_amd", "host", "diploma")
EMUL_DIR = os.path.join(oracle_lib.ROOT, "tests", "emul")
CSRC = os.path.join(oracle_lib.ROOT, "re2-modification_amd", "csrc")

with open(os.path.join(oracle_lib.GOLDEN, "manifest.json")) as f:
    MANIFEST = json.load(f)
NFA_NAMES = [a["name"] for a in MANIFEST["automata"] if a["name"].startswith("nfa_")]

with open(os.path.join(oracle_lib.ROOT, "include", "mfa_hip.h")) as f:
    MAX_BYTES = int(re.search(r"#define\s+MFA_MAX_STRING_BYTES\s+(0x[0-9a-fA-F]+)u", f.read()).group(1), 16)
START, DEAD, INVALID = capi.DFA_STATE_START, capi.DFA_STATE_DEAD, capi.DFA_STATE_INVALID
SPLIT_MIN, CHUNK_MIN, ARENA = 65536, 4096, 131072           # the library's defaults (include/mfa_hip.h)
ROUNDS = 4                                                  # rounds a string in pieces is given in (cuts_for, rounds_of)


def manifest_entry(name):
    return next(a for a in MANIFEST["automata"] if a["name"] == name)


# ---- the host harnesses -----------------------------------------------------------------------------------------------------------------
_built = {}


def emul_exe(name, flags=""):
    """tests/emul/NAME_emul.cpp built by tests/emul/build.sh with `flags` behind the caller's EMUL_FLAGS, once per session, in a temporary
    directory of its own; the compiler is heard only when it fails"""
    if (name, flags) not in _built:
        folder = tempfile.mkdtemp(prefix=name + "_emul_")
        atexit.register(shutil.rmtree, folder, ignore_errors=True)
        exe = os.path.join(folder, name + "_emul")
        env = dict(os.environ, EMUL_FLAGS=(os.environ.get("EMUL_FLAGS", "") + " " + flags).strip())
        p = subprocess.run([os.path.join(EMUL_DIR, "build.sh"), name, exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert p.returncode == 0, "tests/emul/build.sh %s failed:\n%s" % (name, p.stdout)
        _built[(name, flags)] = exe
    return _built[(name, flags)]


def walk_emul_run(exe, path, cap, accel, strings, more=()):
    """walk_emul on one image (more: [image, first string, ...] of further segments): (answers, the counters of the emulation's last
    stderr line; under "fields" what its EMUL_FIELDS line counts per cell, {"c-cm": [n1 .. n9], "c-com", "c-rdm", "b-cm", "b-com", "b-rdm"})"""
    p = subprocess.run([exe, str(path), str(cap), str(accel)] + [str(m) for m in more], input=b"".join(s + b"\n" for s in strings),
                       capture_output=True, env=dict(os.environ, EMUL_FIELDS="1"))
    assert p.returncode == 0, p.stderr.decode()[-400:]
    lines = p.stderr.decode().strip().split("\n")
    stats = {k: int(v) for k, v in re.findall(r"([a-z-]+) (\d+)", lines[-1].split("strings,")[1])}
    words = next(ln for ln in lines if ln.startswith("fields:")).split()[1:]
    stats["fields"] = {words[k]: [int(x) for x in words[k + 1:k + 10]] for k in range(0, len(words), 10)}
    return np.array([int(x) for x in p.stdout.split()], dtype=np.uint8), stats


def write_batch(path, strings):
    """BATCH.bin of the harnesses: u64 n, u64 offsets[n + 1], then offsets[n] bytes; returns oracle_lib.pack(strings)"""
    data, off = oracle_lib.pack(strings)
    path.write_bytes(struct.pack("<Q", len(strings)) + off.astype("<u8").tobytes() + data.tobytes()[:int(off[-1])])
    return data, off


# ---- blobs ------------------------------------------------------------------------------------------------------------------------------
def fixture_blob(name, rev=None):
    """the fixture's image; rev = None: in the direction it was compiled with, 0 or 1: made to scan in that direction"""
    d = image.parse_dump(oracle_lib.load_dump(name))
    if rev is not None:
        d["reversed"] = rev
    return image.to_blob(d)


def blob_of(name, rev):
    """the fixture's image; rev = 1 makes it scan from the end, rev = 0 LEAVES it as compiled (nfa_abb_plain scans from the end either way)"""
    return fixture_blob(name, 1 if rev else None)


def front_end_blob(regex, tmp_path, rev=0, flag="-thompson"):
    """the host front-end's automaton for `regex`; rev = 1 forces the reversed scan on it, as blob_of does for a fixture"""
    p = subprocess.run([DIPLOMA, "-dump", flag], input=regex + "\n", capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode == 0, p.stderr
    d = image.parse_dump(p.stdout)
    if rev:
        d["reversed"] = 1
    return image.to_blob(d)


def k_regex(k):
    """(a|b)*a(a|b)^k: 2^(k+1) state sets in the Thompson compile (+ 2: k = 5 gives 66, 8 gives 514, 14 gives 32 770, 16 gives 131 074)"""
    return "(a|b)*a" + "(a|b)" * k


def table_66(tmp_path, rev=0):
    """(a|b)*a(a|b)^5: 66 state sets, more than a wave"""
    return front_end_blob(k_regex(5), tmp_path, rev)


def table_127(tmp_path, rev=0):
    """127 state sets, the most an LDS table holds"""
    ab = "(a|b)"
    return front_end_blob("(a|b)*(a" + ab * 5 + "|b" + ab * 4 + "a)" + "(c|d)" * 7 + "c*", tmp_path, rev)


# name -> (regex, state sets): the L2 tables of tests/test_dfa_spec_*.py.  t514: the state is the last nine bytes, every guess with nine
# bytes of lookback is right.  counter: (a^300)*, the state is a position modulo 300 and never converges.  prefix: a literal in front of
# t514, so a walk from {start} dies in mid-text.
TABLES = {
    "t514": (k_regex(8), 514),
    "counter": ("(" + "a" * 300 + ")*", None),
    "prefix": ("xyz" + k_regex(8), None),
}


def table_blob(name, tmp_path, rev=0):
    """the host front-end's automaton of TABLES[name]; rev = 1 makes the same automaton scan from the end (the mirrored language)"""
    return front_end_blob(TABLES[name][0], tmp_path, rev)


def rand_regex(rng, depth, cells, allow_mem):
    """A random regex of the README grammar (README.md:11-24): literals, '.', concatenation, alternation in
    parentheses, star on a parenthesised group or a literal, and -- if allow_mem -- {r}:k and &k."""
    if depth <= 0:
        r = rng.random()
        if allow_mem and cells and r < 0.25:
            return "&" + rng.choice(cells)
        return rng.choice("abc.") if r < 0.95 else rng.choice("ab")
    kind = rng.random()
    if kind < 0.35:
        return "".join(rand_regex(rng, depth - 1, cells, allow_mem) for _ in range(rng.randint(2, 3)))
    if kind < 0.55:
        return "(" + "|".join(rand_regex(rng, depth - 1, cells, allow_mem) for _ in range(rng.randint(2, 3))) + ")"
    if kind < 0.75:
        return "(" + rand_regex(rng, depth - 1, cells, allow_mem) + ")*"
    if kind < 0.85 and allow_mem:
        k = rng.choice("12")
        if k not in cells:
            cells.append(k)
        return "{" + rand_regex(rng, depth - 1, cells, False) + "}:" + k
    return rng.choice("abc") + "*"


# ---- batches on the device --------------------------------------------------------------------------------------------------------------
def upload(strings, exact=False):
    """(device bytes, device offsets, host offsets); 64 zero bytes behind the strings, or with exact = True exactly the room the read rule
    of include/mfa_hip.h asks for: whole 16-byte blocks"""
    import torch
    data, off = oracle_lib.pack(strings)
    d_bytes = torch.zeros((len(data) + 15) // 16 * 16 if exact else len(data) + 64, dtype=torch.uint8, device="cuda")
    d_bytes[:len(data)] = torch.from_numpy(data.copy())
    return d_bytes, torch.from_numpy(off.astype(np.int64)).cuda(), off


def filled(n):
    """a result buffer that shows what a call left alone: max(n, 1) bytes of 7"""
    import torch
    return torch.full((max(n, 1),), 7, dtype=torch.uint8, device="cuda")


def match_on_gpu(img, strings, exact=False):
    """one mfa_match_batch call, synchronised: (the strings' result bytes, host offsets)"""
    import torch
    d_bytes, d_off, off = upload(strings, exact)
    res = filled(len(strings))
    img.match_tensors(d_bytes, d_off, res)
    torch.cuda.synchronize()
    return res[:len(strings)].cpu().numpy(), off


def seg_first_of(segments):
    return [0] + [int(x) for x in np.cumsum([len(s) for s in segments])]


def mixed_match(mixed, segments, stream=None):
    import torch
    strings = [s for seg in segments for s in seg]
    d_bytes, d_off, _ = upload(strings)
    res = filled(len(strings))
    mixed.match_tensors(d_bytes, d_off, seg_first_of(segments), res, stream=stream)
    torch.cuda.synchronize()
    return res[:len(strings)].cpu().numpy()


def new_states(n, value=START):
    import torch
    return torch.from_numpy(np.full(max(n, 1), value, dtype=np.uint32).view(np.int32)).cuda()


def states_of(d_states, n):
    return d_states.cpu().numpy().view(np.uint32)[:n].copy()


def feed(img, pieces, d_states, results=True, stream=None):
    """one round: the pieces of all strings through mfa_match_batch_resume; returns the result bytes (None without results)"""
    import torch
    d_bytes, d_off, _ = upload(pieces)
    res = filled(len(pieces)) if results else None
    img.match_tensors_resume(d_bytes, d_off, d_states, res, stream=stream)
    torch.cuda.synchronize()
    return res[:len(pieces)].cpu().numpy() if results else None


def check(got, want, strings, what):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s: %d mismatches, first string %d (len %d) want %d got %d" % (what, bad.size, bad[0], len(strings[bad[0]]), want[bad[0]], got[bad[0]])


def expected_split(off, split_min, chunk_min, arena=ARENA):
    """what mfa_last_dfa_split must report for a batch with these offsets (the formulas of the header)"""
    spans = [(int(b), int(e)) for b, e in zip(off[:-1], off[1:]) if int(e) - int(b) >= split_min]
    if not spans:
        return (0, 0, 0)
    long_bytes = sum(e - b for b, e in spans)
    chunk = max(chunk_min, (long_bytes // arena + 15) // 16 * 16)
    return (len(spans), sum((e - (b & ~15) + chunk - 1) // chunk for b, e in spans), chunk)


# ---- strings ----------------------------------------------------------------------------------------------------------------------------
def rnd(alpha, n, rng):
    return (np.frombuffer(alpha, dtype=np.uint8)[rng.integers(0, len(alpha), size=n)]).tobytes()


def accepted_long(name, n, rng):
    """a string of exactly n bytes (n >= 6000) that the fixture accepts -- all but the four nfa_dot_*, which die on every input tried"""
    if name.startswith(("nfa_abb", "nfa_third")):
        return rnd(b"ab", n - 3, rng) + b"abb"
    if name.startswith("nfa_enum"):
        return rnd(b"abc", n - 3, rng) + b"abc"
    if name.startswith("nfa_star1"):
        return rnd(b"ab", n - 2, rng) + b"ab"
    if name.startswith("nfa_star2"):
        return rnd(b"ab", n - 1, rng) + b"a"
    if name.startswith("nfa_alt3"):
        tail = 5000 + (n & 1)
        words = np.array([[97, 98], [98, 97]], dtype=np.uint8)[rng.integers(0, 2, size=(n - 2 - tail) // 2)]
        return b"ab" + words.tobytes() + b"c" * tail
    if name.startswith("nfa_star4"):
        words = [b"ab", b"c", b"cc", b"abab"]
        idx = rng.integers(0, 4, size=n)
        cum = np.cumsum(np.array([2, 1, 2, 4])[idx])
        m = int(np.searchsorted(cum, n - 1, side="right"))
        body = b"".join(words[i] for i in idx[:m].tolist())
        return body + b"c" * (n - 1 - len(body)) + b"a"
    return rnd(b"ab", n, rng)


def scan_poke(s, k, is_rev):
    """s with the k-th byte IN SCAN ORDER replaced by z (k < 0: from the end of the scan)"""
    i = k if k >= 0 else len(s) + k
    if is_rev:
        i = len(s) - 1 - i
    return s[:i] + b"z" + s[i + 1:]


def short_strings(rng, count=300):
    """the ragged batch of test_gpu_parity.py: test_table_walk_whole_lines"""
    out = []
    for k, ln in enumerate(int(x) for x in rng.integers(0, 700, size=count)):
        t = bytes(rng.choice(list(b"ab" if k % 4 else b"abc."), size=ln).tolist())
        if k % 3 == 0 and ln >= 3:
            t = t[:-3] + b"abb"
        out.append(t)
    return out


def out_offsets(strings):
    at, offs = 0, []
    for s in strings:
        offs.append(at)
        at += len(s)
    return offs


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


# ---- strings in pieces (tests/test_dfa_resume_*.py) -------------------------------------------------------------------------------------
def corpus(name, rev):
    """the strings of strings_for (0 to 20 000 bytes, packed back to back: a start at every offset mod 16), mirrored for the reversed scan,
    with their image and the direction that image scans in (rev = 0 leaves a fixture the direction it was compiled with: nfa_abb_plain
    scans from the end either way)"""
    rng = np.random.default_rng(len(name) * 131 + rev)
    strings = strings_for(name, rng)
    if rev:
        strings = [s[::-1] for s in strings]
    blob = blob_of(name, rev)
    return blob, strings, image.blob_info(blob)["reversed"]


def cuts_for(strings, rng):
    """string k -> its cut points [0, c1, .., len]: 1 to 4 pieces at seeded random points; empty pieces (at either end and in the
    middle) and, in the packed buffer, a cut at every residue mod 16"""
    off = out_offsets(strings)
    cuts = []
    for k, s in enumerate(strings):
        inner = sorted(int(x) for x in rng.integers(0, len(s) + 1, size=k % ROUNDS))
        if inner and len(s) >= 32:                         # the first cut lands on residue k mod 16 of the buffer
            inner[0] = (k % 16 - off[k]) % 16 + 16 * int(rng.integers(0, (len(s) - 16) // 16))
            inner.sort()
        if inner and k % 5 == 0:
            inner[0] = 0                                   # an empty first piece
        if inner and k % 7 == 0:
            inner[-1] = len(s)                             # an empty last piece
        if len(inner) >= 2 and k % 3 == 0:
            inner[1] = inner[0]                            # an empty piece in the middle
        cuts.append([0] + sorted(inner) + [len(s)])
    return cuts


def rounds_of(strings, cuts, rev):
    """ROUNDS lists of (begin, end) per string, relative to the string, IN SCAN ORDER: a reversed automaton is given the last piece
    first.  A string with fewer pieces gets empty ones behind its last"""
    out = []
    for r in range(ROUNDS):
        row = []
        for s, c in zip(strings, cuts):
            pieces = list(zip(c[:-1], c[1:]))
            if rev:
                pieces = pieces[::-1]
            done = 0 if rev else len(s)
            row.append(pieces[r] if r < len(pieces) else (done, done))
        out.append(row)
    return out


def seen_so_far(strings, rounds, r, rev):
    """what string k has been given up to and including round r: a prefix, or for the reversed scan a suffix"""
    return [s[rounds[r][k][0]:] if rev else s[:rounds[r][k][1]] for k, s in enumerate(strings)]


def pieces_against_whole(img, blob, strings, rng, what, oracle_rounds=True):
    """the strings cut as tests/test_dfa_resume_cpu.py cuts them (testlib.cuts_for), fed in ROUNDS rounds in scan order (a string with fewer pieces gets
    empty ones): every round's results against the oracle on what has been given so far; final states against ONE call on the whole
    strings; that call's results against mfa_match_batch and the oracle"""
    is_rev = image.blob_info(blob)["reversed"]
    cuts = cuts_for(strings, rng)
    rounds = rounds_of(strings, cuts, is_rev)
    ora = oracle_lib.OracleImage(blob)
    n = len(strings)
    d_states = new_states(n)
    for r in range(ROUNDS):
        got = feed(img, [s[b:e] for s, (b, e) in zip(strings, rounds[r])], d_states)
        if oracle_rounds or r == ROUNDS - 1:
            want = ora.match(seen_so_far(strings, rounds, r, is_rev))
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, "%s round %d: %d mismatches, first string %d (len %d) want %d got %d" % (what, r, bad.size, bad[0], len(strings[bad[0]]), want[bad[0]], got[bad[0]])
    d_whole = new_states(n)
    whole = feed(img, strings, d_whole)
    assert np.array_equal(states_of(d_states, n), states_of(d_whole, n)), what
    assert np.array_equal(whole, match_on_gpu(img, strings)[0]) and np.array_equal(whole, got), what
    assert int(states_of(d_whole, n).max()) < img.info()["dfa_states"]
    assert img.info()["last_kernel"] == capi.KERNEL_TABLE


# ---- the set walk's corpus (tests/test_nfa_setwalk_*.py) --------------------------------------------------------------------------------
LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 4096]


def accepted_of(name, ln, rng):
    """a string of (about) ln bytes that the fixture's regex accepts, where one of that length exists"""
    pick = lambda alpha, k: bytes(rng.choice(list(alpha), size=max(k, 0)).tolist())
    if name.startswith("nfa_abb"):
        return pick(b"ab", ln - 3) + b"abb"
    if name.startswith("nfa_third"):
        return pick(b"ab", ln - 3) + b"a" + pick(b"ab", 2)
    if name.startswith("nfa_enum"):
        return pick(b"abc", ln - 3) + b"abc"
    if name.startswith("nfa_star1"):
        return pick(b"ab", ln - 2) + b"ab"
    if name.startswith("nfa_star2"):
        return pick(b"ab", ln - 1) + b"a"
    if name.startswith("nfa_star4"):
        body = b"".join(rng.choice([b"ab", b"c", b"cc", b"abab"]) for _ in range(ln // 2 + 1))[:max(ln - 1, 0)]
        while body[-1:] == b"a":
            body = body[:-1]
        return b"c" * (ln - 1 - len(body)) + body + b"a"
    if name.startswith("nfa_alt3"):                        # (ab|b)(ab|ba)*c*
        pairs = max(ln - 2, 0) // 3
        return b"ab" + b"".join(rng.choice([b"ab", b"ba"]) for _ in range(pairs)) + b"c" * max(ln - 2 - 2 * pairs, 0)
    assert name.startswith("nfa_dot")                      # a.c*(b|.a)*
    out = b"a" + pick(b"abcz.", 1) + b"c" * (max(ln - 2, 0) // 4)
    while len(out) < ln:
        out += b"b" if rng.random() < 0.4 or len(out) + 2 > ln else pick(b"abcz", 1) + b"a"
    return out


def setwalk_corpus(name, rev, seed=0, n_golden=440):
    """about 600 strings for a fixture: golden strings (the reference's own answers come with them) and generated ones of LENGTHS and of
    random lengths up to 3000 -- accepted ones, ones rejected by their last byte only, ones that die early.  Packed back to back they
    start at every offset mod 16.  rev: the image is made to scan from the end and the strings are mirrored.
    Returns (blob, strings, golden): golden[k] = the reference's answer for string k, -1 where there is none."""
    rng = np.random.default_rng(len(name) * 257 + rev + 1000 * seed)
    gold_s, gold_b = [], []
    for sset in ("abc7", "rnd", "odd"):
        gold_s += oracle_lib.load_set(sset)
        gold_b += [int(x) for x in oracle_lib.load_bits(name, sset)]
    take = sorted(int(x) for x in rng.choice(len(gold_s), size=n_golden, replace=False))
    strings, golden = [gold_s[k] for k in take], [gold_b[k] for k in take]
    lens = LENGTHS + LENGTHS + [int(x) for x in rng.integers(0, 3001, size=40)] + [int(x) for x in rng.integers(0, 120, size=96)]
    k = 0
    while lens or len({o % 16 for o in out_offsets(strings)}) < 16:
        ln = lens.pop(0) if lens else int(rng.integers(1, 300))
        s = accepted_of(name, ln, rng)[-ln:] if ln else b""      # (shorter than the regex's shortest word: its tail)
        assert len(s) == ln
        if k % 4 == 1 and s:
            s = s[:-1] + b"z"                              # rejected by the last byte only
        if k % 9 == 5 and len(s) > 40:
            s = s[:7] + b"\x00" + s[8:]                    # dies early
        strings.append(s)
        golden.append(-1)
        k += 1
    blob = blob_of(name, rev)
    if rev and not image.blob_info(blob_of(name, 0))["reversed"]:
        strings = [s[::-1] for s in strings]               # the flag makes the same automaton scan from the end: the mirrored language
    return blob, strings, np.array(golden)


def expected(blob, strings, golden):
    """the CPU restatement's answers, held to the reference's own where the corpus has them; both answers must occur"""
    want = oracle_lib.OracleImage(blob).match(strings)
    have = golden >= 0
    assert have.sum() > 300 and np.array_equal(want[have], golden[have].astype(np.uint8))
    assert 0 < int(want.sum()) < len(strings)
    return want


def wide_images(tmp_path):
    """Thompson of nested alternations: more than 32 nodes, more than 64, more than 128, and deep epsilon chains"""
    ab = "(a|b)"
    deep = "a"
    for _ in range(6):
        deep = "((" + deep + "|b)|c)"
    return {"w2": front_end_blob("(a|b)*a" + ab * 4 + "(c|(a|b))*", tmp_path),
            "w4": front_end_blob("((a|b)|(c|a))*" + "((a|b)|c)" * 6, tmp_path),
            "w8": front_end_blob("((a|b)|(c|a))*" + "((a|(b|c))|(c|(a|b)))" * 8, tmp_path),
            "deep": front_end_blob("(" + deep + ")*" + deep, tmp_path, 1)}


def wide_strings(rng, n=300):
    strings = [bytes(rng.choice(list(b"abc"), size=int(ln)).tolist()) for ln in LENGTHS + [int(x) for x in rng.integers(0, 200, size=n - len(LENGTHS))]]
    return strings + [s[:-1] + b"z" for s in strings[3:40]]
