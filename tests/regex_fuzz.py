"""Random memory regexes as TREES, strings sampled from the same tree, and corpora of automaton images made from them by the host
front-end -- TEST INFRASTRUCTURE ONLY, no tests in here (tests/test_walk_fuzz_cpu.py, tests/test_walk_fuzz_gpu.py and the build's warm
list import it).

A tree is a tuple: ("lit", c) | ("dot",) | ("cat", kids) | ("alt", kids) | ("star", kid) | ("mem", kid, k) | ("ref", k).  It renders to the
README grammar ({r}:k initialises cell k with what r read, &k reads it back; an unset cell reads as the empty string), and the sampler
walks it the way a match would: so most strings are accepted or are one edit away from an accepted one, and a long string stays alive to
its end -- what random text never does.  Everything is a pure function of the seed: no clock, no answer decides what is kept."""
import os
import random
import subprocess
import tempfile

from mfa_amd import image
from testlib import DIPLOMA

FLAGS = ("-mfa", "-bnf", "-reverse")
FORCED = "-mfa, scanned from the end"     # the -mfa image with is_reversed set: the second family's directed regexes only
PUMPS = (20, 64, 70, 130, 300, 1000)      # around the region pass's 64-byte minimum, and long enough for chained jumps
MAX_SAMPLE = 20000                        # a sample that grows beyond this is dropped (nested pumped stars)
MAX_VARIED = 6000                         # samples up to this length also yield their three damaged variants
MAX_NODES = 64
MAX_EDGES = 512                           # (a -reverse image of 18 nodes had 3 005 edges: a minute in the restatement, which tries every edge of every live node)
MIN_STRINGS = 20


# ---- the tree ------------------------------------------------------------------------------------------------------------------------
def gen_tree(rng, depth, cells, digits, allow_mem=True, top=False):
    """cells: the cells introduced so far, in generation order (appended to); digits: the cell names this regex may use.  The first
    initialisation takes the LAST of `digits` (the image's cell count is its highest cell), the others any of them."""
    if depth <= 0:
        r = rng.random()
        if allow_mem and cells and r < 0.5:
            return ("ref", rng.choice(cells))
        return ("lit", rng.choice("abc")) if r < 0.92 else ("dot",)
    kind = 0.0 if top else rng.random()                   # (the whole regex: a concatenation, so that a cell set early can be read later)
    if kind < 0.34:
        return ("cat", [gen_tree(rng, depth - 1, cells, digits, allow_mem) for _ in range(rng.randint(2, 3))])
    if kind < 0.50:
        return ("alt", [gen_tree(rng, depth - 1, cells, digits, allow_mem) for _ in range(rng.randint(2, 3))])
    if kind < 0.66:
        return ("star", gen_tree(rng, depth - 1, cells, digits, allow_mem))
    if kind < 0.90 and allow_mem:
        k = digits[-1] if not cells else rng.choice(digits)
        if k not in cells:
            cells.append(k)
        return ("mem", gen_tree(rng, depth - 1, cells, digits, False), k)
    return ("star", ("lit", rng.choice("abc")))


OWN_READ = 0.4                            # share of the second family's initialisations that start with a read of their own cell


def gen_tree2(rng, depth, digits, inside=(), top=False):
    """The second family.  A reference may name ANY cell of `digits`, set or not (a read of an unset cell creates it, empty); the body of
    {..}:k may hold references and other initialisations, never of a cell it is itself inside of (`inside`); and OWN_READ of the
    initialisations are {&k r}:k -- the edge that reads the absent cell k also opens it: the cell is created OPEN."""
    if depth <= 0:
        r = rng.random()
        if r < 0.5:
            return ("ref", rng.choice(digits))
        return ("lit", rng.choice("abc")) if r < 0.92 else ("dot",)
    kind = 0.0 if top else rng.random()
    if kind < 0.30:
        return ("cat", [gen_tree2(rng, depth - 1, digits, inside) for _ in range(rng.randint(2, 3))])
    if kind < 0.44:
        return ("alt", [gen_tree2(rng, depth - 1, digits, inside) for _ in range(rng.randint(2, 3))])
    if kind < 0.60:
        return ("star", gen_tree2(rng, depth - 1, digits, inside))
    if kind < 0.92:
        free = [d for d in digits if d not in inside]
        if not free:
            return ("lit", rng.choice("abc"))
        k = rng.choice(free)
        body = gen_tree2(rng, depth - 1, digits, inside + (k,))
        if rng.random() < OWN_READ:
            body = ("cat", [("ref", k), body])
        return ("mem", body, k)
    return ("star", ("lit", rng.choice("abc")))


def _lits(word):
    return [("lit", c) for c in word]


def star_piece(rng, p, q):
    """a random piece over the letters p, q that holds a star: the X of the directed shapes"""
    return rng.choice([("star", ("lit", p)), ("star", ("cat", _lits(p + q))), ("cat", [("lit", p), ("star", ("lit", p))]),
                       ("star", ("alt", _lits(p + q))), ("cat", [("star", ("lit", p)), ("lit", q)]), ("cat", [("lit", q), ("star", ("lit", p))])])


def directed_trees(rng, ncell):
    """The second family's directed regexes, for every cell k of the limit: a created-open cell is written to and read back with a visible
    outcome (what random trees rarely do), and a reversed scan decides by an is_read mark.  X: a random star-bearing piece, Y and Z: not
    empty, over a letter X does not use.
      write, read back:        ({&k X}:k Y &k Z)*
      from a waiting state:    {aa*}:j &j {&k X}:k Y &k          (a value of one or more bytes is read just before: the state waits)
      a chain two deep:        {&k {&m X}:m Y &m}:k Z &k
      ... from a waiting state: {aa*}:j &j {&k {&m X}:m}:k Y &k &m          (the waiting insertion of the SECOND cell carries the first's open bit)
      read marks (-reverse):   {a*}:k (&k|c) b,   {(ab)*}:k (&k|c) b,   {a*}:k (&k b|&k c|c) b   and   ({a}:k)* c* (&k &m a | &k b)
    Every shape comes once with all its cells among 1..6 (k <= 6: two-word edges) and, where the limit is 9, once with a cell of 7..9 in it
    (three-word edges): that cell is k itself, else the partner j or m of the first three shapes, else a pad {c}:h &h behind the shape
    (the read-mark shapes: a cell that is read and never set is dropped by the normal form -reverse goes through).
    One shape more is no -reverse image but the -mfa image made to scan from the end (FORCED: its strings are the sampled ones turned
    round), because it needs a read of a cell that is never set:  {aa}:k Y (&m b | &k c) Z, Z one letter -- the read attempt of the set cell k
    marks it, the read of the absent cell m (behind it in the node's edge order: the front end lists the last alternative first) recurses, and the mark has to go with the recursion
    (flat_b's `rd`): where it is lost, the state still needs the two bytes of k's value as suffix, and dies in front of Z.
    Returns [(tree, flags)]."""
    out = []
    for wide in ((False, True) if ncell > 6 else (False,)):
        for k in "123456789"[:ncell if wide else min(ncell, 6)]:
            if wide and k < "7":
                others = "789"
            else:
                others = [d for d in "123456789"[:ncell if wide else min(ncell, 6)] if d != k]
            p, q, r = rng.sample("abc", 3)
            x = lambda: star_piece(rng, p, q)
            y = lambda: ("cat", _lits(rng.choice([r, r + r, r + p])))
            own = lambda c: ("mem", ("cat", [("ref", c), x()]), c)
            pad = [("mem", ("lit", "c"), rng.choice("789")), None] if wide and k < "7" else []
            if pad:
                pad[1] = ("ref", pad[0][2])
            j, m = rng.sample(others, 2)
            m2 = rng.choice([d for d in "123456" if d != k]) if pad else rng.choice(others)
            shapes = [
                ("cat", [("star", ("cat", [own(k), y(), ("ref", k), y()]))] + pad) if pad else ("star", ("cat", [own(k), y(), ("ref", k), y()])),
                ("cat", [("mem", ("cat", [("lit", "a"), ("star", ("lit", "a"))]), j), ("ref", j), own(k), y(), ("ref", k)]),
                ("cat", [("mem", ("cat", [("ref", k), own(m), y(), ("ref", m)]), k), y(), ("ref", k)]),
                ("cat", [("mem", ("star", ("lit", "a")), k), ("alt", [("ref", k), ("lit", "c")]), ("lit", "b")] + pad),
                ("cat", [("mem", ("star", ("cat", _lits("ab"))), k), ("alt", [("ref", k), ("lit", "c")]), ("lit", "b")] + pad),
                ("cat", [("mem", ("star", ("lit", "a")), k),
                         ("alt", [("cat", [("ref", k), ("lit", "b")]), ("cat", [("ref", k), ("lit", "c")]), ("lit", "c")]), ("lit", "b")] + pad),
                ("cat", [("star", ("mem", ("lit", "a"), k)), ("star", ("lit", "c")),
                         ("alt", [("cat", [("ref", k), ("ref", m2), ("lit", "a")]), ("cat", [("ref", k), ("lit", "b")])])] + pad),
            ]
            out += [(t, FLAGS) for t in shapes]
            out += [(("cat", [("mem", ("cat", [("lit", "a"), ("star", ("lit", "a"))]), j), ("ref", j), ("mem", ("cat", [("ref", k), own(m)]), k), y(),
                              ("ref", k), ("ref", m)]), FLAGS),
                    (("cat", [("mem", ("cat", _lits("aa")), k), y(),
                              ("alt", [("cat", [("ref", m), ("lit", "b")]), ("cat", [("ref", k), ("lit", "c")])]),
                              ("lit", rng.choice("abc"))]), (FORCED,))]
    return out


def render(t):
    kind = t[0]
    if kind == "lit":
        return t[1]
    if kind == "dot":
        return "."
    if kind == "cat":
        return "".join(render(k) for k in t[1])
    if kind == "alt":
        return "(" + "|".join(render(k) for k in t[1]) + ")"
    if kind == "star":
        return render(t[1]) + "*" if t[1][0] == "lit" else "(" + render(t[1]) + ")*"
    if kind == "mem":
        return "{" + render(t[1]) + "}:" + t[2]
    return "&" + t[1]


def holds_memory(t):
    if t[0] in ("mem", "ref"):
        return True
    if t[0] in ("cat", "alt"):
        return any(holds_memory(k) for k in t[1])
    return t[0] == "star" and holds_memory(t[1])


# ---- strings -------------------------------------------------------------------------------------------------------------------------
class _TooLong(Exception):
    pass


def _sample(t, rng, mem):
    kind = t[0]
    if kind == "lit":
        return t[1]
    if kind == "dot":
        return rng.choice("abc")
    if kind == "cat":
        out = ""
        for k in t[1]:
            out += _sample(k, rng, mem)
            if len(out) > MAX_SAMPLE:
                raise _TooLong()
        return out
    if kind == "alt":
        return _sample(rng.choice(t[1]), rng, mem)
    if kind == "mem":
        mem[t[2]] = _sample(t[1], rng, mem)
        return mem[t[2]]
    if kind == "ref":
        return mem.get(t[1], "")
    r = rng.random()                                      # a star: none, a few, or pumped
    if r < 0.2:
        return ""
    if r < 0.6:
        count, pumped = rng.randint(1, 3), False
    else:
        count, pumped = rng.choice(PUMPS), True
    if pumped and not holds_memory(t[1]) and rng.random() < 0.7:
        body = _sample(t[1], rng, mem)                    # ONE body, repeated: a periodic stretch whose period is the body's length
        if len(body) * count > MAX_SAMPLE:
            raise _TooLong()
        return body * count
    out = ""
    for _ in range(min(count, 100)):
        out += _sample(t[1], rng, mem)
        if len(out) > MAX_SAMPLE:
            raise _TooLong()
    return out


def sample_strings(tree, rng, n_samples):
    """n_samples walks of the tree, each (up to MAX_VARIED bytes) with a replaced byte, a cut prefix and a doubled-back splice;
    bytes objects, non-empty, duplicates dropped, in the order they were made"""
    out, seen = [], set()
    for _ in range(n_samples):
        try:
            s = _sample(tree, rng, {})
        except _TooLong:
            continue
        made = [s]
        if 0 < len(s) <= MAX_VARIED:
            at = rng.randrange(len(s))
            made.append(s[:at] + rng.choice("abc") + s[at + 1:])
            made.append(s[:rng.randint(0, len(s))])
            cut = rng.randint(0, len(s))
            made.append(s[:cut] + s[cut // 2:])
        for m in made:
            if m and m not in seen:
                seen.add(m)
                out.append(m.encode())
    return out


# ---- corpora -------------------------------------------------------------------------------------------------------------------------
def front_end_blob(regex, flag, cwd):
    """the image `diploma -dump FLAG` builds, or None where the front end refuses the regex"""
    p = subprocess.run([DIPLOMA, "-dump", flag], input=regex + "\n", capture_output=True, text=True, cwd=cwd)
    if p.returncode != 0:
        return None
    try:
        return image.blob_from_dump(p.stdout)
    except image.ImageError:
        return None


class Corpus(list):
    first_directed = None                     # family 2: the index of the first image of a directed regex (they are the corpus's last)


def corpus(seed, n_regex, ncell, n_samples=40, family=1):
    """[(regex, flag, blob, strings)]: n_regex random regexes that hold '{' or '&', regex i limited to the first 1 + i % ncell cells, each
    as -mfa, -bnf and -reverse image with the strings sampled from its tree.  Skipped, by rule: what the front end refuses, images that are
    not memory automata, images of more than MAX_NODES nodes or MAX_EDGES edges, regexes with fewer than MIN_STRINGS distinct strings.
    family 1: gen_tree.  family 2: gen_tree2, and behind the random regexes the directed ones of directed_trees(ncell), under the same rules."""
    rng = random.Random((0x5EED0000 if family == 1 else 0x5EED1000) + 1000 * ncell + seed)
    out, kept = Corpus(), 0
    with tempfile.TemporaryDirectory() as tmp:              # (the front end leaves drawings in its working directory)
        def images_of(tree, regex, flags=FLAGS):
            strings = sample_strings(tree, rng, n_samples)
            if len(strings) < MIN_STRINGS:
                return
            for flag in flags:
                blob = front_end_blob(regex, "-mfa" if flag == FORCED else flag, tmp)
                if blob is None:
                    continue
                if flag == FORCED:
                    blob = blob[:12] + (1).to_bytes(4, "little") + blob[16:]          # (the header's is_reversed: include/mfa_image_format.h)
                    strings = [s[::-1] for s in strings]
                info = image.blob_info(blob)
                if info["kind"] != image.KIND_MFA or info["n_nodes"] > MAX_NODES or info["n_edges"] > MAX_EDGES:
                    continue
                out.append((regex, flag, blob, strings))

        while kept < n_regex:
            digits = "123456789"[:1 + kept % ncell]
            tree = gen_tree(rng, rng.randint(2, 4), [], digits, top=True) if family == 1 else gen_tree2(rng, rng.randint(2, 4), digits, top=True)
            regex = render(tree)
            if "{" not in regex and "&" not in regex:
                continue
            kept += 1
            images_of(tree, regex)
        if family == 2:
            out.first_directed = len(out)
            for tree, flags in directed_trees(rng, ncell):
                images_of(tree, render(tree), flags)
    return out


# ---- what the table builder makes of an image: the fields of created cells ---------------------------------------------------------------
def table_fields(blob):
    """{"c-cm": [n1 .. n9], "c-com", "c-rdm", "b-cm", "b-com", "b-rdm"}: per cell, the effective edges of the image's walk tables that hold
    the cell in cm (created on the way), com (created open) and rdm (read marks), in the vnodes' waiting lists (c) and byte-class lists (b):
    the flattening of csrc/walk_tables.cpp (flat_b, flat_c over the reachable vnodes) restated, so that a corpus can be CHOSEN by these
    fields where no compiler is at hand.  tests/test_walk_fuzz2_cpu.py holds it against what tests/emul/walk_emul counts in the tables
    themselves (EMUL_FIELDS), image by image."""
    import struct
    f = struct.unpack_from("<10I", blob, 0)
    n_nodes, n_edges, start, finish = f[4], f[5], f[6], f[7]
    begin = struct.unpack_from("<%dI" % (n_nodes + 1), blob, 40)
    edges = [struct.unpack_from("<BBHI", blob, 40 + 4 * (n_nodes + 1) + 8 * e) for e in range(n_edges)]
    out_of = [edges[begin[n]:begin[n + 1]] for n in range(n_nodes)]

    def digit(e):
        return e[0] - 0x31 if not e[1] & image.EDGE_EPS and 0x31 <= e[0] <= 0x39 else -1

    def opens(e, d):
        return (e[3] >> (2 * (d + 1))) & 3 == image.ACT_OPEN

    def opens_of(e):
        return sum(1 << c for c in range(9) if opens(e, c))

    classes = sorted({e[0] for e in edges if not e[1] & image.EDGE_EPS and e[0] != 0x2e}) + [-1]
    n = {name: [0] * 9 for name in ("c-cm", "c-com", "c-rdm", "b-cm", "b-com", "b-rdm")}

    def count(which, cm, com, rdm):
        for c in range(9):
            n[which + "-cm"][c] += (cm >> c) & 1
            n[which + "-com"][c] += (com >> c) & 1
            n[which + "-rdm"][c] += (rdm >> c) & 1

    def qualifies(node, mask):
        return any(not e[1] & image.EDGE_EPS and (digit(e) < 0 or (mask >> digit(e)) & 1) for e in out_of[node])

    def flat_b(node, fm, cm, com, rd, byte, targets):
        for e in out_of[node]:
            if e[1] & image.EDGE_EPS:
                continue
            d = digit(e)
            if d >= 0 and not (fm >> d) & 1:
                if e[2] != finish:
                    flat_b(e[2], fm | 1 << d, cm | 1 << d, com | (1 << d if opens(e, d) else 0), rd, byte, targets)
                continue
            if e[0] == 0x2e or (byte >= 0 and byte == e[0]):
                count("b", cm, com, rd)
                targets.append((e[2], fm | opens_of(e)))
            elif d >= 0:
                count("b", cm, com, rd)
                targets.append((e[2], fm | opens_of(e)))
                rd |= 1 << d

    def flat_c(node, fm, cm, com, targets):
        for e in out_of[node]:
            d = digit(e)
            if d < 0 or (fm >> d) & 1 or e[2] == finish:
                continue
            fm2, cm2, com2 = fm | 1 << d, cm | 1 << d, com | (1 << d if opens(e, d) else 0)
            flat_c(e[2], fm2, cm2, com2, targets)
            if qualifies(e[2], fm2):
                count("c", cm2, com2, 0)
                targets.append((e[2], fm2))

    seen, todo = {(start, 0)}, [(start, 0)]
    while todo:
        node, mask = todo.pop()
        targets = []
        for byte in classes:
            flat_b(node, mask, 0, 0, 0, byte, targets)
        flat_c(node, mask, 0, 0, targets)
        for t in targets:
            if t not in seen:
                seen.add(t)
                todo.append(t)
    return n


# ---- the GPU tests' fixed corpus -------------------------------------------------------------------------------------------------------
GPU_SEED, GPU_REGEXES, GPU_NCELL, GPU_SAMPLES = 0, 90, 9, 100
GPU_BATCH, GPU_BATCH_BYTES = 330, 900 * 1024

_gpu = None


def _gpu_batch(regex, strings):
    """about GPU_BATCH of an image's strings, never a multiple of 64, under GPU_BATCH_BYTES in all, shuffled; None: too few"""
    rng = random.Random(len(regex) + 31 * len(strings))
    batch, total = [], 0
    for s in strings:
        if len(batch) < GPU_BATCH and total + len(s) <= GPU_BATCH_BYTES:
            batch.append(s)
            total += len(s)
    if len(batch) < GPU_BATCH // 2:                         # (a regex of few distinct strings: the mixed batches need 131 of an image)
        return None
    if len(batch) % 64 == 0:
        batch.pop()
    rng.shuffle(batch)
    return batch


def gpu_corpus():
    """24 images of corpus(seed 0), in this order: 8 forward -mfa images of 1-3 cells, 4 of 4-9 cells (three of at most 6 cells, then one of
    7 or more), 6 -bnf, 6 -reverse with is_reversed == 1 -- of each kind the first ones the corpus holds that have a cell.  A dict per image: regex, flag,
    blob, cells, strings (about GPU_BATCH of them, never a multiple of 64, under GPU_BATCH_BYTES in all, shuffled)."""
    global _gpu
    if _gpu is not None:
        return _gpu
    want = {"few": 8, "mid": 3, "wide": 1, "bnf": 6, "rev": 6}
    got = {k: [] for k in want}
    for regex, flag, blob, strings in corpus(GPU_SEED, GPU_REGEXES, GPU_NCELL, GPU_SAMPLES):
        info = image.blob_info(blob)
        if flag == "-mfa":
            kind = None if info["reversed"] else "few" if info["n_cells"] <= 3 else "mid" if info["n_cells"] <= 6 else "wide"
        elif flag == "-bnf":
            kind = "bnf"
        else:
            kind = "rev" if info["reversed"] == 1 else None
        if kind is None or info["n_cells"] == 0 or len(got[kind]) >= want[kind]:      # (no cell: -bnf drops the cells nothing reads)
            continue
        batch = _gpu_batch(regex, strings)
        if batch is None:
            continue
        got[kind].append({"regex": regex, "flag": flag, "blob": blob, "cells": info["n_cells"], "edges": info["n_edges"], "strings": batch})
    for k in want:
        assert len(got[k]) == want[k], "the corpus holds %d %s images, %d wanted" % (len(got[k]), k, want[k])
    _gpu = got["few"] + got["mid"] + got["wide"] + got["bnf"] + got["rev"]
    return _gpu


GPU_SAMPLES2 = 200                        # (the directed regexes have fewer distinct strings per sample)
_gpu2 = None


def gpu_corpus2():
    """16 images of corpus(seed 0, family 2), in this order: 6 forward -mfa images of 1, 2 .. 6 cells whose tables hold a cell created open
    (com), 4 of 7-9 cells with com, 3 -bnf, 3 -reverse with is_reversed == 1 whose tables hold read marks (rdm) -- of each kind the first
    ones the corpus holds, the directed regexes' images in front of the random ones (their strings are accepted or rejected BY the created
    cell).  A dict per image as in gpu_corpus(), and "fields": table_fields(blob)."""
    global _gpu2
    if _gpu2 is not None:
        return _gpu2
    want = {"narrow": 6, "wide": 4, "bnf": 3, "rev": 3}
    got = {k: [] for k in want}
    whole = corpus(GPU_SEED, GPU_REGEXES, GPU_NCELL, GPU_SAMPLES2, family=2)
    for regex, flag, blob, strings in whole[whole.first_directed:] + whole[:whole.first_directed]:
        info = image.blob_info(blob)
        fields = table_fields(blob)
        com = any(fields["c-com"]) or any(fields["b-com"])
        if flag == "-mfa":
            kind = None if info["reversed"] or not com else "narrow" if info["n_cells"] <= 6 else "wide"
            if kind == "narrow" and info["n_cells"] in [im["cells"] for im in got["narrow"]]:
                kind = None                                 # (one image per cell count: a mixed launch per count)
        elif flag == "-bnf":
            kind = "bnf"
        elif flag == "-reverse":
            kind = "rev" if info["reversed"] == 1 and any(fields["b-rdm"]) else None
        else:
            kind = None
        if kind is None or info["n_cells"] == 0 or len(got[kind]) >= want[kind]:
            continue
        batch = _gpu_batch(regex, strings)
        if batch is None:
            continue
        got[kind].append({"regex": regex, "flag": flag, "blob": blob, "cells": info["n_cells"], "edges": info["n_edges"], "strings": batch,
                          "reversed": info["reversed"], "fields": fields})
    for k in want:
        assert len(got[k]) == want[k], "the second corpus holds %d %s images, %d wanted" % (len(got[k]), k, want[k])
    got["narrow"].sort(key=lambda im: im["cells"])
    _gpu2 = got["narrow"] + got["wide"] + got["bnf"] + got["rev"]
    return _gpu2


def jit_source_size(blob):
    """bytes of the source the generator writes for this automaton's specialised kernel (what its compile time goes with), or None where
    the generator refuses the automaton.  No compiler runs: the library is given one that fails at once (MFA_HIPCC) and a cache directory of
    its own (MFA_JIT_CACHE), where it leaves the source it generated."""
    from mfa_amd import capi
    saved = {k: os.environ.get(k) for k in ("MFA_HIPCC", "MFA_JIT_CACHE")}
    try:
        with tempfile.TemporaryDirectory() as tmp:
            os.chmod(tmp, 0o700)
            os.environ["MFA_HIPCC"] = "/bin/false"
            os.environ["MFA_JIT_CACHE"] = tmp
            img = capi.Image(blob)
            err = os.dup(2)                                 # (the library reports the failed compiler run on stderr: expected here)
            null = os.open(os.devnull, os.O_WRONLY)
            os.dup2(null, 2)
            try:
                if img.specialize() is False:
                    return None
            except capi.MfaError:
                pass
            finally:
                os.dup2(err, 2)
                os.close(err)
                os.close(null)
                img.close()
            left = [f for f in os.listdir(tmp) if f.endswith(".failed.hip")]
            assert len(left) == 1, left
            return os.path.getsize(os.path.join(tmp, left[0]))
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_spec = None


def specialised_six():
    """the six images of gpu_corpus() with at most 50 edges whose generated kernels have the smallest source (ties: corpus order): the ones
    the build compiles ahead (warm_specialised_kernels) and test_walk_fuzz_gpu walks with the specialised engine"""
    global _spec
    if _spec is None:
        sized = []
        for k, im in enumerate(gpu_corpus()):
            if im["edges"] <= 50:
                size = jit_source_size(im["blob"])
                if size is not None:
                    sized.append((size, k))
        assert len(sized) >= 6, "only %d images of the GPU corpus can have a specialised kernel" % len(sized)
        _spec = [gpu_corpus()[k] for _, k in sorted(sized)[:6]]
    return _spec


SPEC2_KINDS = {
    "com in a byte-class list": lambda im: any(im["fields"]["b-com"]),
    "com in a waiting list": lambda im: any(im["fields"]["c-com"]),       # (the generated kernel's phase-C insertion)
    "scanned from the end": lambda im: im["reversed"] == 1,
    "four cells or more": lambda im: im["cells"] >= 4,
}
_spec2 = None


def specialised_eight():
    """the eight images of gpu_corpus2() with at most 50 edges whose generated kernels have the smallest source (ties: corpus order) -- and
    where these miss one of SPEC2_KINDS, the largest of them that no kind needs gives way to the smallest image of that kind: the ones the
    build compiles ahead and test_walk_fuzz_gpu walks with the specialised engine.  [(source bytes, image)]"""
    global _spec2
    if _spec2 is None:
        sized = []
        for k, im in enumerate(gpu_corpus2()):
            if im["edges"] <= 50:
                size = jit_source_size(im["blob"])
                if size is not None:
                    sized.append((size, k))
        sized.sort()
        assert len(sized) >= 8, "only %d images of the second GPU corpus can have a specialised kernel" % len(sized)
        c = gpu_corpus2()
        chosen, rest = sized[:8], sized[8:]
        for name, has in SPEC2_KINDS.items():
            if not any(has(c[k]) for _, k in chosen):
                new = next((sk for sk in rest if has(c[sk[1]])), None)
                assert new is not None, "no image of the second GPU corpus that can have a specialised kernel has: " + name
                needed = lambda sk: any(h(c[sk[1]]) and sum(h(c[k]) for _, k in chosen) == 1 for h in SPEC2_KINDS.values())
                chosen.remove(max(sk for sk in chosen if not needed(sk)))
                rest.remove(new)
                chosen = sorted(chosen + [new])
        _spec2 = [(size, c[k]) for size, k in chosen]
    return _spec2
