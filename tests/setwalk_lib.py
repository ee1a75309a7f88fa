"""What the tests of the set walk share (tests/test_nfa_set_{resume,split,wave,wave_resume,wave_split}_{cpu,gpu}.py and the set-walk parts
of tests/test_nfa_fuzz_*.py): the runs of the host harnesses tests/emul/nfa_set_{resume,split,wave,wave_resume,wave_split}_emul.cpp (built
by testlib.emul_exe) with their input files and their output, the images and strings the tests walk, the cuts they feed, and the records of
mfa_match_batch_resume_set (the lane record, LANE_WORDS words) and mfa_match_batch_resume_set_wide (the wide record, WIDE_WORDS words) on
the host and on the device -- TEST INFRASTRUCTURE ONLY: no tests, no fixtures, no marks in here.  torch is imported where it is used, so
that collecting the CPU tests needs no GPU."""
import random
import struct
import subprocess
import sys

import numpy as np

import nfa_fuzz
import oracle_lib
from mfa_amd import capi, image
from testlib import (DIPLOMA, LENGTHS, MAX_BYTES, ROUNDS, accepted_of, blob_of, cuts_for, front_end_blob, k_regex, out_offsets, rounds_of, upload, wide_strings,
                     write_batch)

LANE_WORDS, WIDE_WORDS = capi.SET_STATE_WORDS, capi.SET_STATE_WIDE_WORDS        # a record: tag, reserved[3], then 8 or 64 node words
START, LIVE, INVALID = capi.SET_STATE_START, capi.SET_STATE_LIVE, capi.SET_STATE_INVALID
LANE_MAX_NODES, WAVE_MAX_NODES = 256, 2048
CHUNKS = (16, 32, 64)
LOOKBACKS = (0, 8, 256)
REPAIR_ROUNDS = (0, 1, 3, 8)                       # repair-round counts of the split path (testlib.ROUNDS is another thing: rounds of pieces)
N_ROUNDS = 3                                       # rounds the wide records are fed in (three_rounds, fixed_cuts)
# (a^300)* has 303 nodes, more than a lane image holds (256): COUNTER is the longest round one that fits, 253 nodes, W = 8
COUNTER = "(" + "a" * 250 + ")*"
COUNTER300 = "(" + "a" * 300 + ")*"
PREFIX = "xyz(a|b)*abb"                            # a literal prefix in front of a loop: a walk from {start} dies in mid-text
PREFIX_WIDE = "xyz(a|b)*a" + "(a|b)" * 52          # ... in front of a loop of more than 256 nodes
EDGE_LENGTHS = [1023, 1024, 1025, 2049]            # the edges of a fetch round (64 blocks of 16 bytes), and two rounds and a byte
FIXED_LENGTHS = (0, 1, 15, 16, 17, 1023, 1024, 1025)
RAW_NODES = (257, 288, 512, 513, 1024, 1025, 2047, 2048)
# seeds for which the ORACLE answers both ways on the sampled strings (a scan of seeds 0 to 7 on the CPU restatement alone; odd seeds scan
# from the end); six labels keep the live sets tens of nodes wide
RAW_SEEDS = {257: (0, 1, 3), 288: (2, 3, 7), 512: (0, 1, 3), 513: (0, 1, 3), 1024: (2, 4, 5), 1025: (0, 1, 5), 2047: (0, 1, 3), 2048: (2, 3, 6)}
RAW_LABELS = 6
GUARD = 0x5a5a5a5a
# the counts of an "ok" line of nfa_set_split_emul, and of nfa_set_wave_split_emul's split mode
LANE_SPLIT_KEYS = ("W", "checks", "rewalked", "serial_strings", "serial_bytes", "home_nodes", "home_guesses")
WAVE_SPLIT_KEYS = LANE_SPLIT_KEYS + ("invalid_ends",)
COUNT_KEYS = ("rewalked", "serial_strings", "serial_bytes")


def mask_words(n_nodes):
    """the node words a lane image's masks take"""
    return 1 if n_nodes <= 32 else 2 if n_nodes <= 64 else 4 if n_nodes <= 128 else 8


def words_of(n_nodes):
    """the node words (lanes) a wave image's masks take"""
    return (n_nodes + 31) // 32


# ---- harness runs -----------------------------------------------------------------------------------------------------------------------
# run: what runs the command line instead of subprocess.run -- it returns the finished process, or None for "refused", which the runner
# returns as it is
def _finished(cmd, run=None):
    p = subprocess.run(cmd, capture_output=True) if run is None else run(cmd)
    assert p is None or p.returncode == 0, p.stderr.decode()[-1200:]
    return p


def _files(tmp_path, blob, strings=None):
    """[a.blob, batch.bin] written"""
    (tmp_path / "a.blob").write_bytes(blob)
    if strings is None:
        return [str(tmp_path / "a.blob")]
    write_batch(tmp_path / "batch.bin", strings)
    return [str(tmp_path / "a.blob"), str(tmp_path / "batch.bin")]


def _states_file(tmp_path, states):
    (tmp_path / "states.bin").write_bytes(np.ascontiguousarray(states, dtype="<u4").tobytes())
    return str(tmp_path / "states.bin")


def _digits(text):
    return np.frombuffer(text, dtype=np.uint8) - ord("0")


def ok_line(stdout, at=0):
    """the numbers of the "ok ..." line that is line `at` of a harness's output"""
    f = stdout.split(b"\n")[at].split()
    assert f[0] == b"ok", f
    return tuple(int(x) for x in f[1:])


def tables_line(stdout):
    """(table words, W, depth) of a wave harness's leading "tables WORDS W DEPTH" line"""
    f = stdout.split(b"\n")[0].split()
    assert f[0] == b"tables", f
    return tuple(int(x) for x in f[1:])


def split_blocks(stdout, combos, keys):
    """the "ok COUNTS / digits" blocks of a split harness, one per combination: a list of (combination, counts by key, result digits)"""
    lines = stdout.split(b"\n")
    out = []
    for i, combo in enumerate(combos):
        w = lines[2 * i].split()
        assert w[0] == b"ok" and len(w) == 1 + len(keys), lines[2 * i]
        out.append((combo, dict(zip(keys, (int(x) for x in w[1:]))), _digits(lines[2 * i + 1])))
    return out


def pieces_output(stdout, n_rounds, n, words, queued=False, tables=False):
    """the output of a `pieces` mode -- a "tables" line if `tables`; one line per round, its result digits and, if `queued`, a count behind
    them; one line per string, its final record in hex: (one array of digits per round, the counts, the records as an [n, words] array)"""
    lines = stdout.split(b"\n")[1 if tables else 0:]
    digits, counts = [], []
    for ln in lines[:n_rounds]:
        f = ln.split()                                                    # (no string: the digits are empty)
        digits.append(_digits(f[0] if len(f) == 1 + queued else b""))
        counts.append(int(f[-1]) if queued else None)
    assert all(len(d) == n for d in digits)
    recs = np.array([[int(w, 16) for w in ln.split()] for ln in lines[n_rounds:n_rounds + n]], dtype=np.uint32).reshape(n, words)
    return digits, counts, recs


def write_round(path, rnd):
    """ROUND.bin of the wave harnesses -- u64 n, u64 total, u64 offsets[n + 1], then `total` bytes -- for the list of a round's pieces as
    one call gets them, or a raw_round; returns n"""
    if isinstance(rnd, tuple) and rnd[0] == "raw":
        off, data = rnd[1], rnd[2]
    else:
        off, data = [0] + [int(x) for x in np.cumsum([len(p) for p in rnd])], b"".join(rnd)
    path.write_bytes(struct.pack("<QQ", len(off) - 1, len(data)) + np.asarray(off, dtype="<u8").tobytes() + data)
    return len(off) - 1


def raw_round(offsets, data):
    """a round given by its offsets alone (they may point outside `data`)"""
    return ("raw", [int(x) for x in offsets], bytes(data))


def write_cuts(path, rounds):
    """CUTS.bin of nfa_set_resume_emul: u64 rounds, then per round and string (u64 begin, u64 end), relative to the string"""
    path.write_bytes(struct.pack("<Q", len(rounds)) + np.array([[p for p in row] for row in rounds], dtype="<u8").reshape(-1).tobytes())


def _round_files(tmp_path, rounds):
    """(the ROUND.bin files of the rounds, written; the number of strings, the same in all of them)"""
    paths, counts = [], set()
    for r, rnd in enumerate(rounds):
        paths.append(str(tmp_path / ("round%d.bin" % r)))
        counts.add(write_round(tmp_path / ("round%d.bin" % r), rnd))
    assert len(counts) == 1
    return paths, counts.pop()


def run_lane_pieces(exe, tmp_path, blob, strings, rounds, states=None):
    """nfa_set_resume_emul pieces: rounds[r][k] = (begin, end) of string k's piece in round r, relative to the string.  Returns (one
    array of result digits per round, the final records as an [n, LANE_WORDS] array of uint32)"""
    write_cuts(tmp_path / "cuts.bin", rounds)
    more = [] if states is None else [_states_file(tmp_path, states)]
    p = _finished([exe, "pieces"] + _files(tmp_path, blob, strings) + [str(tmp_path / "cuts.bin")] + more)
    digits, _, recs = pieces_output(p.stdout, len(rounds), len(strings), LANE_WORDS)
    return digits, recs


def run_wide_pieces(exe, tmp_path, blob, rounds, states=None):
    """nfa_set_wave_resume_emul pieces: rounds[r] is the list of the strings' pieces of round r, as one call gets them, or a raw_round.
    Returns ((table words, W, depth), one array of result digits per round, the final records as an [n, WIDE_WORDS] array of uint32)"""
    paths, n = _round_files(tmp_path, rounds)
    p = _finished([exe, "pieces"] + _files(tmp_path, blob) + ["-" if states is None else _states_file(tmp_path, states)] + paths)
    digits, _, recs = pieces_output(p.stdout, len(rounds), n, WIDE_WORDS, tables=True)
    return tables_line(p.stdout), digits, recs


def run_wide_split_pieces(exe, tmp_path, blob, rounds, chunk, lookback, repair_rounds, split_min, states=None):
    """nfa_set_wave_split_emul pieces, on the rounds of run_wide_pieces.  Returns (one array of result digits per round, the count of
    queued pieces per round, the final records as an [n, WIDE_WORDS] array of uint32)"""
    paths, n = _round_files(tmp_path, rounds)
    p = _finished([exe, "pieces"] + _files(tmp_path, blob) + ["-" if states is None else _states_file(tmp_path, states)]
                  + [str(chunk), str(lookback), str(repair_rounds), str(split_min)] + paths)
    tables_line(p.stdout)
    return pieces_output(p.stdout, len(rounds), n, WIDE_WORDS, queued=True, tables=True)


def run_lane_table(exe, tmp_path, blob, strings):
    """nfa_set_resume_emul table: [strings, states, W] of its "ok" line"""
    return list(ok_line(_finished([exe, "table"] + _files(tmp_path, blob, strings)).stdout))


def run_wide_table(exe, tmp_path, blob, strings):
    """nfa_set_wave_resume_emul table: ((table words, W, depth), strings, states)"""
    p = _finished([exe, "table"] + _files(tmp_path, blob, strings))
    return (tables_line(p.stdout),) + ok_line(p.stdout, 1)


def run_step(exe, tmp_path, blob):
    """nfa_set_wave_emul step: (states, classes, W, depth) of its "ok" line"""
    return ok_line(_finished([exe, "step"] + _files(tmp_path, blob)).stdout)


def run_match(exe, tmp_path, blob, strings, run=None):
    """nfa_set_wave_emul match: one result byte per string"""
    p = _finished([exe, "match"] + _files(tmp_path, blob, strings), run)
    return None if p is None else _digits(p.stdout.strip())


def _split_lists(chunks, lookbacks, repair_rounds):
    """(the three lists as the harnesses take them, their combinations in the order of the output: chunks outermost)"""
    return [",".join(str(x) for x in v) for v in (chunks, lookbacks, repair_rounds)], [(c, lb, r) for c in chunks for lb in lookbacks for r in repair_rounds]


def run_lane_split(exe, tmp_path, blob, strings, chunks, lookbacks, repair_rounds, mode="one", run=None):
    """nfa_set_split_emul on every combination of the three lists: split_blocks with LANE_SPLIT_KEYS"""
    lists, combos = _split_lists(chunks, lookbacks, repair_rounds)
    p = _finished([exe] + _files(tmp_path, blob, strings) + lists + [mode], run)
    return None if p is None else split_blocks(p.stdout, combos, LANE_SPLIT_KEYS)


def run_wave_split(exe, tmp_path, blob, strings, chunks, lookbacks, repair_rounds, depth=None, run=None):
    """nfa_set_wave_split_emul split on every combination of the three lists: split_blocks with WAVE_SPLIT_KEYS.  depth: the stacks'
    slots, instead of the tables' own"""
    lists, combos = _split_lists(chunks, lookbacks, repair_rounds)
    p = _finished([exe, "split"] + _files(tmp_path, blob, strings) + lists + ([str(depth)] if depth is not None else []), run)
    return None if p is None else split_blocks(p.stdout, combos, WAVE_SPLIT_KEYS)


def tables_in_lds(tables):
    """whether the four stacks and the tables fit the 64 KiB a block may take, from the harness's "tables WORDS W DEPTH" line"""
    words, _, depth = tables
    return (4 * depth + words) * 4 <= 65536


# ---- images -----------------------------------------------------------------------------------------------------------------------------
def k_blob(k, tmp_path, rev=0):
    """(a|b)*a(a|b)^k, Thompson: the set is fixed by the last k + 1 bytes"""
    return front_end_blob(k_regex(k), tmp_path, rev)


def eps_chain(d):
    """the most nodes on one path of epsilon edges of a parsed dump (what image_host.cpp: nfa_eps_chain counts)"""
    nodes, memo = d["nodes"], {}
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 4 * len(nodes) + 100))

    def go(u):
        if u not in memo:
            memo[u] = 1 + max([go(to) for lab, to, _ in nodes[u]["edges"] if lab is None] or [0])
        return memo[u]

    try:
        return max(go(u) for u in range(len(nodes)))
    finally:
        sys.setrecursionlimit(old)


def k_for(lo, hi, tmp_path):
    """the smallest k whose Thompson compile of k_regex(k) has more than lo nodes; asserted to have at most hi.  (5 k + 9 nodes today:
    found by asking the front-end, not by that slope)"""
    nodes = lambda k: image.blob_info(front_end_blob(k_regex(k), tmp_path))["n_nodes"]
    k = max(1, lo // 5 - 3)
    while nodes(k) <= lo:
        k += 1
    assert lo < nodes(k) <= hi
    return k


def deep_wide_dump(tmp_path):
    """nested alternations in the style of testlib.wide_images()["deep"], more of them: the parsed dump, made to scan from the end"""
    deep = "a"
    for _ in range(14):
        deep = "((" + deep + "|b)|c)"
    p = subprocess.run([DIPLOMA, "-dump", "-thompson"], input="(" + deep + ")*" + deep + deep + "\n", capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode == 0, p.stderr
    d = image.parse_dump(p.stdout)
    d["reversed"] = 1
    return d


def wide_regex_images(tmp_path):
    """name -> (blob, alphabet, min_len): k_regex Thompson images in (256, 512], (512, 1024] and (1024, 2048] nodes, the first also
    scanning from the end, and the deep one (more than 256 nodes AND an epsilon chain beyond the lane kernel's 49 nodes).  alphabet and
    min_len are for regex_strings: (a|b)*a(a|b)^k accepts nothing with a `c` and nothing shorter than k + 1 bytes"""
    out = {}
    for name, lo, hi in (("k_512", 256, 512), ("k_1024", 512, 1024), ("k_2048", 1024, 2048)):
        k = k_for(lo, hi, tmp_path)
        out[name] = (front_end_blob(k_regex(k), tmp_path), b"ab", k + 1)
        if lo == 256:
            out[name + "_rev"] = (front_end_blob(k_regex(k), tmp_path, 1), b"ab", k + 1)
    d = deep_wide_dump(tmp_path)
    assert len(d["nodes"]) > LANE_MAX_NODES and eps_chain(d) > 49
    out["deep"] = (image.to_blob(d), b"abc", 0)
    return out


def raw_image(n_nodes, seed):
    """a raw random image (nfa_fuzz.random_image: forward epsilon edges only, so no cycle; `finish` drawn anywhere), scanning from the end
    for odd seeds: (dict, blob)"""
    rng = random.Random(1000003 * n_nodes + seed)
    d = nfa_fuzz.random_image(rng, n_nodes, RAW_LABELS, rev=seed & 1)
    return d, image.to_blob(d)


# ---- strings ----------------------------------------------------------------------------------------------------------------------------
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


def pack_every_offset(strings, filler):
    """the strings with fillers (filler(k) -> a short string) put between them until, packed back to back, they start at every offset
    mod 16"""
    out = list(strings)
    k = 0
    while len({o % 16 for o in out_offsets(out)}) < 16:
        out.append(filler(k))
        k += 1
        assert k < 400
    return out


def regex_strings(rng, alphabet=b"abc", min_len=0):
    """testlib.wide_strings (its `c` made a `b` for an alphabet without one) plus LENGTHS plus EDGE_LENGTHS over the alphabet, plus, for
    an image that accepts nothing below min_len bytes, 60 strings of up to 300 bytes more than that; a start at every offset mod 16"""
    pick = lambda ln: bytes(rng.choice(list(alphabet), size=int(ln)).tolist())
    strings = wide_strings(rng)
    if b"c" not in alphabet:
        strings = [s.replace(b"c", b"b") for s in strings]
    strings += [pick(ln) for ln in LENGTHS + EDGE_LENGTHS]
    if min_len:
        strings += [pick(min_len + int(x)) for x in rng.integers(0, 300, size=60)]
    strings = pack_every_offset(strings, lambda k: pick(1 + k % 7))
    assert {o % 16 for o in out_offsets(strings)} == set(range(16)) and set(LENGTHS + EDGE_LENGTHS) <= {len(s) for s in strings}
    return strings


def raw_strings(d, seed):
    """strings for a raw image, drawn from the automaton (nfa_fuzz's sampler: random text never accepts there): the sampler's own batch,
    and one string of every length of LENGTHS and EDGE_LENGTHS where the automaton has a loop to pump; None when nothing pumps.  In the
    order the image reads them (mirrored for a reversed scan); a start at every offset mod 16."""
    rng = random.Random(77 * seed + len(d["nodes"]))
    E, start, finish = nfa_fuzz.edges_by_rank(d)
    got = nfa_fuzz.sample_strings(E, start, finish, rng, 0)
    if got is None:
        return None
    strings = list(got[0])
    sm = nfa_fuzz.Sampler(E, start, finish, rng)
    for ln in LENGTHS + EDGE_LENGTHS:
        s, cur = [], frozenset([sm.w.start])        # exactly ln bytes that keep the set alive (the sampler's own strings stop at LONG_MAX)
        while len(s) < ln:
            nb = sm.next_byte(cur)
            if nb is None:
                return None
            s.append(nb[0])
            cur = nb[1]
        strings.append(bytes(s))
    strings = pack_every_offset(strings, lambda k: strings[k % 16][:1 + k % 7])
    assert {o % 16 for o in out_offsets(strings)} == set(range(16)) and set(LENGTHS + EDGE_LENGTHS) <= {len(s) for s in strings}
    return [s[::-1] for s in strings] if d["reversed"] else strings


def raw_corpus(node_counts=RAW_NODES, per=3):
    """[(name, blob, strings, want)] over the node counts and the first `per` of their RAW_SEEDS, and the number dropped: an image is
    dropped when nothing pumps or when the ORACLE does not answer both ways on its strings -- a filter on the reference alone"""
    out, dropped = [], 0
    for n_nodes in node_counts:
        for seed in RAW_SEEDS[n_nodes][:per]:
            d, blob = raw_image(n_nodes, seed)
            strings = raw_strings(d, seed)
            want = None if strings is None else np.asarray(oracle_lib.OracleImage(blob).match(strings)).copy()
            if want is None or not 0 < int(want.sum()) < len(strings):
                dropped += 1
                continue
            want.setflags(write=False)
            out.append(("raw_%d_seed%d" % (n_nodes, seed), blob, strings, want))
    return out, dropped


_raw = {}


def raw_corpus_once(node_counts=RAW_NODES, per=3):
    """raw_corpus, made once per session and left unchanged"""
    if (node_counts, per) not in _raw:
        _raw[(node_counts, per)] = raw_corpus(node_counts, per)
    return _raw[(node_counts, per)]


# ---- cuts -------------------------------------------------------------------------------------------------------------------------------
# a round of cuts: (begin, end) per string, relative to the string; rounds come in scan order
def whole(strings):
    """one round: every string whole"""
    return [[(0, len(s)) for s in strings]]


def pieces_of(strings, row):
    return [s[b:e] for s, (b, e) in zip(strings, row)]


def piece_rounds(blob, strings, rng):
    """(testlib.ROUNDS rounds of cut strings as testlib.rounds_of gives them, whether the image scans from the end)"""
    is_rev = image.blob_info(blob)["reversed"]
    return rounds_of(strings, cuts_for(strings, rng), is_rev), is_rev


def three_rounds(blob, strings, rng):
    """(N_ROUNDS rounds, whether the image scans from the end): piece_rounds with the pieces of its last two rounds, which lie side by
    side, fed as one"""
    four, is_rev = piece_rounds(blob, strings, rng)
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


# ---- records ----------------------------------------------------------------------------------------------------------------------------
def record(words, tag, nodes=(), reserved=(0, 0, 0)):
    """one record of `words` words: tag, reserved[3], then the node words (node v: bit v & 31 of word v >> 5); nodes: the words from the
    first, or a dict word -> value"""
    row = np.zeros(words, dtype=np.uint32)
    row[0] = tag
    row[1:4] = reserved
    for k, w in (nodes.items() if isinstance(nodes, dict) else enumerate(nodes)):
        row[4 + k] = w
    return row


def check_records_are_clean(recs, n_nodes, words):
    """what the contract promises of every record on return: tag LIVE or INVALID, reserved zero, nothing at or beyond the image's mask
    width, nothing for a node the image lacks, an INVALID record's nodes zero"""
    assert recs.shape[1] == words
    W = mask_words(n_nodes) if words == LANE_WORDS else words_of(n_nodes)
    assert set(np.unique(recs[:, 0])) <= {LIVE, INVALID}
    assert not recs[:, 1:4].any() and not recs[:, 4 + W:].any()
    have = np.zeros(words - 4, dtype=np.uint32)
    for v in range(n_nodes):
        have[v >> 5] |= np.uint32(1 << (v & 31))
    assert not (recs[:, 4:] & ~have).any()
    assert not recs[recs[:, 0] == INVALID, 4:].any()


def sticky_case():
    """the records and the two rounds of the sticky-error test, for the 303-node counter (which scans forward), shared with the GPU test:
    (rows, rounds as raw_round, the strings the good records have been given after each round, indices of the errors, index of the
    dead record, indices of the good records)"""
    piece = b"a" * 150
    rec = lambda *a: record(WIDE_WORDS, *a)
    rows = [rec(2), rec(START), rec(INVALID), rec(LIVE, [1], (0, 5, 0)), rec(START, [], (1, 0, 0)), rec(START, [0xdeadbeef] * 64),
            rec(LIVE, {9: 1 << 15}), rec(LIVE, {0: 1, 10: 1}), rec(START), rec(LIVE, {0: 1, 63: 1 << 31}), rec(LIVE), rec(START)]
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
        assert list(recs[dead]) == [LIVE] + [0] * (WIDE_WORDS - 1), what
        assert (recs[good, 0] == LIVE).all() and recs[good, 4:].any(axis=1).all() and np.array_equal(recs[good[0]], recs[good[1]]) and np.array_equal(recs[good[0]], recs[good[2]]), what
        check_records_are_clean(recs, 303, WIDE_WORDS)
    assert list(ora.match(given[1])) == [1, 1, 1] and list(ora.match(given[0])) == [0, 0, 0]


# ---- on the device ------------------------------------------------------------------------------------------------------------------------
def new_records(n, words, rows=None):
    """n zeroed records of `words` words on the device (every string at its start), or the given [n, words] array, with a guard quarter
    of 16 bytes in front and behind: the whole buffer; the records are records_view(buf, n, words)"""
    import torch
    host = np.full((max(n, 1) * words + 8,), GUARD, dtype=np.uint32)
    host[4:4 + max(n, 1) * words] = 0 if rows is None else np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1)
    return torch.from_numpy(host.view(np.int32).copy()).cuda()


def records_view(buf, n, words):
    view = buf[4:4 + max(n, 1) * words]
    assert view.data_ptr() % 16 == 0
    return view


def records_of(buf, n, words):
    """the records, after a look at the guard quarters"""
    host = buf.cpu().numpy().view(np.uint32)
    assert (host[:4] == GUARD).all() and (host[4 + max(n, 1) * words:] == GUARD).all(), "a record word outside the records"
    return host[4:4 + n * words].reshape(n, words).copy()


def call_records(img, d_bytes, d_off, buf, n, words, results=True, stream=None):
    """one mfa_match_batch_resume_set call (words = LANE_WORDS) or mfa_match_batch_resume_set_wide call (WIDE_WORDS) on uploaded
    pieces, NOT synchronised: the guarded result buffer (64 bytes of 7 on either side), or None"""
    import torch
    res = torch.full((n + 128,), 7, dtype=torch.uint8, device="cuda") if results else None
    call = img.match_tensors_resume_set if words == LANE_WORDS else img.match_tensors_resume_set_wide
    call(d_bytes, d_off, records_view(buf, n, words), res[64:64 + n] if results else None, stream=stream)
    return res


def results_of(res, n):
    host = res.cpu().numpy()
    assert (host[:64] == 7).all() and (host[64 + n:] == 7).all(), "a result byte outside the results"
    return host[64:64 + n].copy()


def feed_records(img, pieces, buf, words, results=True, stream=None):
    """one round: the pieces of all strings through call_records, the batch in exactly the room the read rule asks for; returns the
    result bytes (None without results)"""
    import torch
    d_bytes, d_off, _ = upload(pieces, exact=True)
    res = call_records(img, d_bytes, d_off, buf, len(pieces), words, results, stream)
    torch.cuda.synchronize()
    return results_of(res, len(pieces)) if results else None
