"""Random memory-less automata and strings sampled from them, for the memory-less engines (tests/test_nfa_fuzz_cpu.py,
tests/test_nfa_fuzz_gpu.py) -- TEST INFRASTRUCTURE ONLY: no tests, no fixtures, no marks in here.

Two families.  The first is raw: random_image draws nodes, ranks and edges directly, with labels from all 255 bytes but '.', so that an
image has up to 200 byte classes, labels of 0x80 and above, 0x00 and 0x0a, and letter edges to lower ranks -- where the reference's step
(nodes in rank order, an edge to a visited node skipped even when it is a letter edge, a node marked after its edges) parts from the
textbook one.  The second is what callers produce: testlib.rand_regex without memory through `diploma -dump` with every compile.

step() and accepts() restate that step in plain Python on a rank-numbered edge list: the sampler walks it, and it is a restatement of its
own beside image_host.cpp (Stepper), nfa_set_core.h and oracle/mfa_oracle.c.

corpus(seed) draws until every line of LINES holds an image per scan direction; an image is kept only if the oracle answers 1 on 10-90 % of
its strings -- a filter on the reference alone.  What the library refuses is counted, never hidden.

set_corpus(seed) is the corpus for the tests that walk EVERY image as a node set: the same images, and the direction twin of each whose
lane tables lie beyond LDS (set_placement, from `nfa_set_emul table`), so that both placements are walked in both directions."""
import os
import random
import subprocess
import tempfile

import numpy as np

import oracle_lib
import testlib
from mfa_amd import capi, image

DOT = 0x2e
SPECIAL = (0x00, 0x0a, 0x7f, 0x80, 0xff)
NODES = (2, 3, 5, 8, 12, 20, 33, 40, 65, 70, 129, 130)
LABELS = (0, 1, 2, 3, 4, 5, 7, 8, 12, 40, 200)          # 0: only '.'
MAX_DEG, P_EPS, P_DOT = 3, 0.25, 0.1
PROBE_LIMIT = 3000                                      # an image of more state sets than this is only ever walked as a node set
LONG_MIN, LONG_MAX = 256, 3000
BATCH_MAX, BATCH_MIN, BATCH_BYTES = 330, 165, 1 << 20
REGEX_FLAGS = ("-thompson", "-glushkov", "-ssnf", "")
REFUSAL_CAP = 0.05


# ---- the reference's step, restated ---------------------------------------------------------------------------------------------------
def edges_by_rank(img):
    """the image dict's edges numbered by rank: E[r] = [(label, target rank)], label None for an epsilon edge, else a byte ('.' = DOT
    matches every byte); returns (E, start rank, finish rank)"""
    ranks = [nd["rank"] for nd in img["nodes"]]
    E = [None] * len(ranks)
    for nd in img["nodes"]:
        E[nd["rank"]] = [(None if lab is None else lab[0], ranks[to]) for lab, to, _ in nd["edges"]]
    return E, ranks[img["start"]], ranks[img["finish"]]


def step(E, finish, cur, letter):
    """one step of the reference on the set `cur` of ranks (letter < 0: the final pass): the live nodes in rank order; an edge whose target
    has been visited is skipped, letter edge or not; a node is marked visited after its edges.  Returns a frozenset."""
    nxt, vis = set(), set()

    def visit(node):
        if letter < 0 and node == finish:
            nxt.add(node)
        else:
            for lab, to in E[node]:
                if to in vis:
                    continue
                if lab is None:
                    visit(to)
                elif letter >= 0 and (lab == DOT or lab == letter):
                    nxt.add(to)
        vis.add(node)

    for v in sorted(cur):
        if v not in vis:
            visit(v)
    return frozenset(nxt)


class Walker:
    """step() with a memory: (set, letter) -> set, per image (the step is a pure function of both)"""

    def __init__(self, E, start, finish):
        self.E, self.start, self.finish = E, start, finish
        self.memo = {}

    def step(self, cur, letter):
        key = (cur, letter)
        if key not in self.memo:
            self.memo[key] = step(self.E, self.finish, cur, letter)
        return self.memo[key]

    def accepting(self, cur):
        return self.finish in self.step(cur, -1)

    def accepts(self, s, rev):
        """the reference's answer for the string: bytes in scan order, the early end when the set is empty"""
        cur = frozenset([self.start])
        for b in (reversed(s) if rev else s):
            cur = self.step(cur, b)
            if not cur:
                return 0
        return 1 if self.accepting(cur) else 0


def accepts(E, start, finish, s, rev=0):
    return Walker(E, start, finish).accepts(s, rev)


# ---- the raw family -------------------------------------------------------------------------------------------------------------------
def label_pool(rng, n_labels):
    """n_labels distinct bytes, none of them '.'; 0x00, 0x0a, 0x7f, 0x80 and 0xff among them when there is room for all five (a smaller
    pool is drawn from those five and five others)"""
    others = [b for b in range(256) if b != DOT and b not in SPECIAL]
    if n_labels >= len(SPECIAL):
        return list(SPECIAL) + rng.sample(others, n_labels - len(SPECIAL))
    return rng.sample(list(SPECIAL) + rng.sample(others, len(SPECIAL)), n_labels)


def random_image(rng, n_nodes, n_labels, p_dot=P_DOT, max_deg=MAX_DEG, p_eps=P_EPS, rev=0):
    """a dict for image.to_blob: kind nfa, start = list index 0, a random finish, ranks a random permutation; epsilon edges from a lower to
    a higher list index only (no cycle), letter edges anywhere; labels drawn from the pool without replacement (the pool is shuffled
    again when it runs out), '.' with probability p_dot"""
    ranks = list(range(n_nodes))
    rng.shuffle(ranks)
    pool = label_pool(rng, n_labels)
    bag = []
    nodes = []
    for i in range(n_nodes):
        edges = []
        for _ in range(max(rng.randint(1, max_deg), rng.randint(1, max_deg))):
            if i + 1 < n_nodes and rng.random() < p_eps:
                edges.append((None, rng.randrange(i + 1, n_nodes), {}))
                continue
            if not pool or rng.random() < p_dot:
                lab = DOT
            else:
                if not bag:
                    bag = pool[:]
                    rng.shuffle(bag)
                lab = bag.pop()
            edges.append((bytes([lab]), rng.randrange(n_nodes), {}))
        nodes.append({"rank": ranks[i], "edges": edges})
    return {"kind": image.KIND_NFA, "reversed": rev, "start": 0, "finish": rng.randrange(n_nodes), "nodes": nodes}


def regex_image(rng, flag, rev=0):
    """(regex, the parsed dump of `diploma -dump FLAG`) for a random regex without memory; None if the compile is no memory-less image"""
    regex = ""
    while len(regex) < 3:
        regex = testlib.rand_regex(rng, rng.randint(2, 3), [], False)
    p = subprocess.run([testlib.DIPLOMA, "-dump"] + ([flag] if flag else []), input=regex + "\n", capture_output=True, text=True, cwd=tempfile.gettempdir())
    assert p.returncode == 0, (regex, flag, p.stderr)
    d = image.parse_dump(p.stdout)
    if d["kind"] != image.KIND_NFA:
        return None
    if rev:
        d["reversed"] = 1
    return regex, d


# ---- strings --------------------------------------------------------------------------------------------------------------------------
def class_map(E):
    """byte -> class as the library numbers them: a class per literal label in order of first appearance (rank by rank, edge by edge),
    one more for every other byte"""
    cls = {}
    for edges in E:
        for lab, _ in edges:
            if lab is not None and lab != DOT and lab not in cls:
                cls[lab] = len(cls)
    return cls


class Sampler:
    def __init__(self, E, start, finish, rng):
        self.w = Walker(E, start, finish)
        self.rng = rng
        self.labels = sorted(class_map(E))
        self.others = [b for b in range(256) if b != DOT and b not in set(self.labels)]
        self.closure = {}

    def offers(self, cur):
        """the labels on the letter edges that a textbook closure of `cur` reaches: more than the reference's step follows"""
        if cur not in self.closure:
            seen, todo, labs = set(cur), list(cur), set()
            while todo:
                for lab, to in self.w.E[todo.pop()]:
                    if lab is None:
                        if to not in seen:
                            seen.add(to)
                            todo.append(to)
                    else:
                        labs.add(lab)
            self.closure[cur] = sorted(labs)
        return self.closure[cur]

    def byte_for(self, lab):
        """a '.' edge: a byte outside the labels, 0x80 and above included, sometimes the byte '.' itself"""
        if lab != DOT:
            return lab
        r = self.rng.random()
        if r < 0.15 or not self.others:
            return DOT
        if r < 0.5:
            high = [b for b in self.others if b >= 0x80]
            if high:
                return self.rng.choice(high)
        return self.rng.choice(self.others)

    def next_byte(self, cur):
        """(byte, set) that keeps the set alive, or None"""
        labs = self.offers(cur)[:]
        self.rng.shuffle(labs)
        for lab in labs[:6]:
            b = self.byte_for(lab)
            nxt = self.w.step(cur, b)
            if nxt:
                return b, nxt
        return None

    def sample(self, target):
        """one string IN SCAN ORDER of about `target` bytes that keeps the set alive to its end; pumped when target >= LONG_MIN: the live
        set after every byte is recorded, and when one recurs the bytes between are a loop, repeated up to the target.  Most samples end
        where the automaton accepts, if it does anywhere near.  None: no string that long (nothing recurs)."""
        cur = frozenset([self.w.start])
        out, seen, good = [], {cur: 0}, 0 if self.w.accepting(cur) else -1
        pumped = target < LONG_MIN
        while len(out) < target + 40:
            if len(out) >= target and (good == len(out) or good < 0 and len(out) >= target + 39):
                break
            nb = self.next_byte(cur)
            if nb is None:
                break
            out.append(nb[0])
            cur = nb[1]
            if not pumped and cur in seen:
                loop = out[seen[cur]:]
                out += loop * max(0, (target - len(out)) // len(loop))
                pumped = True
            seen.setdefault(cur, len(out))
            if self.w.accepting(cur):
                good = len(out)
        if target >= LONG_MIN and len(out) < LONG_MIN:
            return None
        if 0 <= good < len(out) and len(out) - good < 40 and self.rng.random() < 0.8:
            out = out[:good]
        return bytes(out[:LONG_MAX])

    def variants(self, s):
        """in scan order: the last byte changed, cut at a random point, one byte poked to a byte of another class"""
        if not s:
            return []
        cls = class_map(self.w.E)
        other = lambda b: self.rng.choice([x for x in self.labels + self.others[:3] + [DOT] if cls.get(x, -1) != cls.get(b, -1)] or [b ^ 1])
        k = self.rng.randrange(len(s))
        return [s[:-1] + bytes([other(s[-1])]), s[:self.rng.randrange(len(s))], s[:k] + bytes([other(s[k])]) + s[k + 1:]]


def sample_strings(E, start, finish, rng, rev, n_short=48, n_long=16):
    """A batch for the image, or None when nothing pumps.  n_long pumped strings of LONG_MIN to LONG_MAX bytes, n_short short ones, each
    with its three variants, and the empty string; packed back to back, pumped string k starts at offset k mod 16 (a cut variant of the
    needed length goes in front of it); BATCH_MIN to BATCH_MAX strings, never a multiple of 64, under BATCH_BYTES.  Mirrored when the
    image scans from the end.  Returns (strings, the Walker that sampled them)."""
    sm = Sampler(E, start, finish, rng)
    longs = []
    for k in range(n_long):
        s = sm.sample(rng.choice((LONG_MIN, 300, 700, 1500, LONG_MAX - 50)) if k >= 2 else (LONG_MIN, LONG_MAX - 50)[k])
        if s is None:
            return None
        longs.append(s)
    rest = [b""]
    for s in longs[:6]:
        rest += sm.variants(s)
    for _ in range(n_short):
        s = sm.sample(rng.choice((0, 1, 2, 3, 5, 8, 15, 16, 17, 31, 33, 64, 100)))
        rest += [s] + sm.variants(s)
    rng.shuffle(rest)
    out, at = [], 0
    for k, s in enumerate(longs):
        for _ in range(rng.randint(0, len(rest) // max(len(longs) - k, 1))):
            out.append(rest.pop())
            at += len(out[-1])
        fill = (k - at) % 16
        if fill:
            out.append(s[:fill])                                # a cut variant of the length that moves the begin where it has to be
            at += fill
        assert at % 16 == k % 16
        out.append(s)
        at += len(s)
    out += rest
    out = out[:BATCH_MAX - 1]
    if len(out) % 64 == 0:
        out.append(longs[0][:7])
    assert BATCH_MIN <= len(out) <= BATCH_MAX and len(out) % 64 and sum(len(s) for s in out) < BATCH_BYTES
    return ([s[::-1] for s in out] if rev else out), sm.w


# ---- corpora --------------------------------------------------------------------------------------------------------------------------
def probe(blob):
    """capi.Image(blob).info() with the tabulation held to PROBE_LIMIT state sets (beyond it: dfa_states 0, as for any set-walk image; the
    tests create their images with the limit at its default and get the same count below it); None: the library refuses the image"""
    old = os.environ.get("MFA_DFA_STATE_LIMIT")
    os.environ["MFA_DFA_STATE_LIMIT"] = str(PROBE_LIMIT)
    os.environ.pop("MFA_NFA_SETWALK", None)
    try:
        img = capi.Image(blob)
    except capi.MfaError as e:
        assert e.code == capi.ERR_UNSUPPORTED, e
        return None
    finally:
        if old is None:
            del os.environ["MFA_DFA_STATE_LIMIT"]
        else:
            os.environ["MFA_DFA_STATE_LIMIT"] = old
    info = img.info()
    img.close()
    return info


def packed(info):
    """make_packed's rule (csrc/kernels.hip): at most 8 state sets and 8 byte classes"""
    return 1 <= info["dfa_states"] <= 8 and info["byte_classes"] <= 8


def mask_words(info):
    n = info["n_nodes"]
    return 1 if n <= 32 else 2 if n <= 64 else 4 if n <= 128 else 8


def states_between(lo, hi):
    return lambda i: lo <= i["dfa_states"] <= hi


# what the tests count on: every line needs an image per scan direction (tests/test_nfa_fuzz_*.py assert it from info() alone)
LINES = dict(
    [("packed, %d literal classes" % k, (lambda k: lambda i: packed(i) and i["byte_classes"] - 1 == k)(k)) for k in range(5)]
    + [("packed-eligible, 5 or more literal classes", lambda i: packed(i) and i["byte_classes"] - 1 >= 5),
       ("9-55 state sets", states_between(9, 55)), ("56-64 state sets", states_between(56, 64)), ("65-127 state sets", states_between(65, 127)),
       ("128-254 state sets", states_between(128, 254)), ("255 state sets or more", states_between(255, 1 << 20))]
    + [("set walk, %d mask words" % w, (lambda w: lambda i: mask_words(i) == w)(w)) for w in (1, 2, 4, 8)])
ONCE = {"40 byte classes or more": lambda i: i["byte_classes"] >= 40, "200 byte classes or more": lambda i: i["byte_classes"] >= 200}
N_REGEX_IMAGES = 8
MAX_DRAWS = 6000


def line_counts(images):
    """line -> [images that scan forward, from the end]; ONCE lines -> a count"""
    out = {name: [sum(1 for im in images if has(im["info"]) and im["info"]["is_reversed"] == rev) for rev in (0, 1)] for name, has in LINES.items()}
    out.update({name: sum(1 for im in images if has(im["info"])) for name, has in ONCE.items()})
    return out


class Corpus(list):
    """the images, and what was drawn for them: drawn, refused (by mfa_image_create; refused_what says which), unbalanced, unpumped"""
    drawn = refused = unbalanced = unpumped = 0

    def __init__(self):
        super().__init__()
        self.refused_what = []


def drawn(d, corpus, what):
    """(info, blob) of a drawn image, counted; None: mfa_image_create refuses it"""
    blob = image.to_blob(d)
    corpus.drawn += 1
    info = probe(blob)
    if info is None:
        corpus.refused += 1
        corpus.refused_what.append(what)
        return None
    return info, blob


def entry(d, blob, info, rng, what, corpus):
    """the image as a corpus entry, or None: nothing pumps, or the oracle answers one way on more than 90 % of the strings"""
    E, start, finish = edges_by_rank(d)
    got = sample_strings(E, start, finish, rng, d["reversed"])
    if got is None:
        corpus.unpumped += 1
        return None
    strings, walker = got
    want = np.asarray(oracle_lib.OracleImage(blob).match(strings)).copy()
    want.setflags(write=False)
    if not 0.1 <= want.mean() <= 0.9:
        corpus.unbalanced += 1
        return None
    labels = sorted(class_map(E))
    return {"what": what, "dict": d, "blob": blob, "info": info, "strings": strings, "want": want, "E": E, "start": start, "finish": finish,
            "walker": walker, "labels": labels, "high_label": any(b >= 0x80 for b in labels),
            "down_edge": any(lab is not None and to < r for r, edges in enumerate(E) for lab, to in edges)}


_corpora = {}


def corpus(seed):
    """Draws over the grids NODES x LABELS, both scan directions in turn, until every line of LINES has an image per direction and the ONCE
    lines one; then N_REGEX_IMAGES regex-derived images, every compile in both directions.  Deterministic in the seed."""
    if seed in _corpora:
        return _corpora[seed]
    rng = random.Random(7919 * seed + 17)
    out = Corpus()
    lacking = lambda info: [n for n, has in LINES.items() if has(info) and not any(has(im["info"]) and im["info"]["is_reversed"] == info["is_reversed"] for im in out)] + \
                           [n for n, has in ONCE.items() if has(info) and not any(has(im["info"]) for im in out)]
    full = lambda: all(min(v) > 0 if isinstance(v, list) else v > 0 for v in line_counts(out).values())
    grid = []
    while not full():
        assert out.drawn < MAX_DRAWS, "the lines are not met after %d draws: %r" % (out.drawn, line_counts(out))
        if not grid:
            grid = [(n, m) for n in NODES for m in LABELS]
            rng.shuffle(grid)
        n_nodes, n_labels = grid.pop()
        rev = out.drawn & 1
        d = random_image(rng, n_nodes, n_labels, rev=rev)
        got = drawn(d, out, "raw, %d nodes, %d labels" % (n_nodes, n_labels))
        if got is None or not lacking(got[0]):
            continue
        im = entry(d, got[1], got[0], rng, "raw, %d nodes, %d labels, seed %d draw %d" % (n_nodes, n_labels, seed, out.drawn), out)
        if im is not None:
            out.append(im)
    k = 0
    while sum(1 for im in out if im["what"].startswith("regex")) < N_REGEX_IMAGES:
        assert out.drawn < MAX_DRAWS
        flag, rev = REGEX_FLAGS[k % 4], (k // 4) & 1
        k += 1
        got = regex_image(rng, flag, rev)
        if got is None:
            continue
        regex, d = got
        fin = drawn(d, out, "regex %r %s" % (regex, flag or "(no flag)"))
        if fin is None or fin[0]["dfa_states"] == 0:
            continue
        im = entry(d, fin[1], fin[0], rng, "regex %r %s" % (regex, flag or "(no flag)"), out)
        if im is not None:
            out.append(im)
    _corpora[seed] = out
    return out


def cpu_corpus(seed):
    return corpus(seed)


def gpu_corpus():
    """the one corpus of the GPU tests: seed 0, made once per session"""
    return corpus(0)


# ---- the corpus of the set walk: every image, and both table placements in both directions -----------------------------------------------
SET_LDS_BYTES = 65536                                   # kSetLdsMax (csrc/nfa_set.h)
_tables, _set_corpora = {}, {}


def direction_twin(im):
    """the same automaton scanning the other way, on the same strings mirrored: an entry like corpus()'s, its info probed anew and its
    answers asked of the oracle anew (they are the original's when the oracle is right: check_set_lines)"""
    d = dict(im["dict"], reversed=0 if im["dict"]["reversed"] else 1)
    blob = image.to_blob(d)
    info = probe(blob)
    assert info is not None and info["is_reversed"] == d["reversed"], im["what"]
    strings = [s[::-1] for s in im["strings"]]
    want = np.asarray(oracle_lib.OracleImage(blob).match(strings)).copy()
    want.setflags(write=False)
    return dict(im, what=im["what"] + ", direction flipped", dict=d, blob=blob, info=info, strings=strings, want=want, twin_of=im)


def set_tables(im):
    """(WORDS, W, DEPTH, CLASSES) of the image's lane tables, from `nfa_set_emul table`; None: the image gets no set-walk tables"""
    if im["blob"] not in _tables:
        with tempfile.TemporaryDirectory(prefix="nfa_fuzz_") as folder:
            path = os.path.join(folder, "a.blob")
            with open(path, "wb") as f:
                f.write(im["blob"])
            p = subprocess.run([testlib.emul_exe("nfa_set"), "table", path], capture_output=True)
        assert p.returncode in (0, 3), p.stderr.decode()[-400:]
        f = p.stdout.split()
        assert p.returncode == 3 or (f[0] == b"tables" and len(f) == 5), p.stdout
        _tables[im["blob"]] = None if p.returncode == 3 else tuple(int(x) for x in f[1:])
    return _tables[im["blob"]]


def set_placement(im):
    """"lds" or "l2": where the lane kernels read the image's tables, by set_lds_of's rule (csrc/nfa_set.h) on the harness's figures: the
    256 stacks and the tables fit 64 KiB, or the tables are read through L2; None: no set-walk tables"""
    t = set_tables(im)
    if t is None:
        return None
    words, _, depth, _ = t
    return "lds" if (depth * 256 + words) * 4 <= SET_LDS_BYTES else "l2"


def set_corpus(seed):
    """corpus(seed), unchanged and in its order, and behind it the direction twin of every image whose tables lie beyond LDS: such images
    are rare, and the draws need not find one per direction.  A list, made once per seed."""
    if seed not in _set_corpora:
        c = list(corpus(seed))
        _set_corpora[seed] = c + [direction_twin(im) for im in c if set_placement(im) == "l2"]
    return _set_corpora[seed]


def set_id(k, im):
    """the test id of image k of a set corpus: mask width, direction, placement"""
    return "%d-W%d-%s-%s" % (k, mask_words(im["info"]), "rev" if im["info"]["is_reversed"] else "fwd", set_placement(im))


def check_set_lines(c):
    """a set corpus is what the set-walk tests count on -- from the harness's table figures and the oracle alone: an image per mask width
    and direction, and per direction one with tables in LDS and one with tables through L2.  A seed without an image beyond LDS fails."""
    have = {(mask_words(im["info"]), im["info"]["is_reversed"], set_placement(im)) for im in c}
    assert all(p is not None for _, _, p in have), "an image without set-walk tables"
    for w in (1, 2, 4, 8):
        for rev in (0, 1):
            assert any(h[:2] == (w, rev) for h in have), "no image of %d mask words, reversed %d" % (w, rev)
    for rev in (0, 1):
        for place in ("l2", "lds"):
            assert any(h[1:] == (rev, place) for h in have), "no image with tables in %s, reversed %d: %r" % (place, rev, sorted(have))
    for im in c:
        t = set_tables(im)
        assert t[1] == mask_words(im["info"]) and t[3] == im["info"]["byte_classes"], (im["what"], t)
        if "twin_of" in im:
            assert np.array_equal(im["want"], im["twin_of"]["want"]), im["what"]
            assert len(im["strings"]) % 64 != 0 and [len(s) for s in im["strings"]] == [len(s) for s in im["twin_of"]["strings"]]


def report_set(c, seed):
    print("nfa fuzz seed %d, set corpus: %d images" % (seed, len(c)))
    for k, im in enumerate(c):
        if set_placement(im) == "l2":
            print("  tables through L2: %s -- %d words, W %d, depth %d, %d classes (%s)" % ((set_id(k, im),) + set_tables(im) + (im["what"],)))


def report(c, seed):
    print("nfa fuzz seed %d: %d images of %d drawn, %d refused, %d unbalanced, %d without a loop to pump" % (seed, len(c), c.drawn, c.refused, c.unbalanced, c.unpumped))
    for what in c.refused_what:
        print("  refused: %s" % what)
    for name, v in line_counts(c).items():
        print("  %-45s %s" % (name, v))
    print("  %-45s %d of %d" % ("a label of 0x80 or above", sum(im["high_label"] for im in c), len(c)))
    print("  %-45s %d of %d" % ("a letter edge to a lower rank", sum(im["down_edge"] for im in c), len(c)))


def check_lines(c):
    """the corpus is what the tests count on -- from info() and the oracle alone"""
    counts = line_counts(c)
    for name, v in counts.items():
        assert (min(v) if isinstance(v, list) else v) >= 1, (name, v)
    assert 3 * sum(im["high_label"] for im in c) >= len(c) and 3 * sum(im["down_edge"] for im in c) >= len(c)
    assert c.refused <= REFUSAL_CAP * c.drawn, (c.refused, c.drawn)
    for im in c:
        n = len(im["strings"])
        assert BATCH_MIN <= n <= BATCH_MAX and n % 64 != 0 and sum(len(s) for s in im["strings"]) < BATCH_BYTES and max(len(s) for s in im["strings"]) <= LONG_MAX
        assert 0.1 <= im["want"].mean() <= 0.9, im["what"]
        off = testlib.out_offsets(im["strings"])
        assert {o % 16 for o, s in zip(off, im["strings"]) if len(s) >= LONG_MIN} == set(range(16)), im["what"]
