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


def corpus(seed, n_regex, ncell, n_samples=40):
    """[(regex, flag, blob, strings)]: n_regex random regexes that hold '{' or '&', regex i limited to the first 1 + i % ncell cells, each
    as -mfa, -bnf and -reverse image with the strings sampled from its tree.  Skipped, by rule: what the front end refuses, images that are
    not memory automata, images of more than MAX_NODES nodes or MAX_EDGES edges, regexes with fewer than MIN_STRINGS distinct strings."""
    rng = random.Random(0x5EED0000 + 1000 * ncell + seed)
    out, kept = [], 0
    with tempfile.TemporaryDirectory() as tmp:              # (the front end leaves drawings in its working directory)
        while kept < n_regex:
            digits = "123456789"[:1 + kept % ncell]
            tree = gen_tree(rng, rng.randint(2, 4), [], digits, top=True)
            regex = render(tree)
            if "{" not in regex and "&" not in regex:
                continue
            kept += 1
            strings = sample_strings(tree, rng, n_samples)
            if len(strings) < MIN_STRINGS:
                continue
            for flag in FLAGS:
                blob = front_end_blob(regex, flag, tmp)
                if blob is None:
                    continue
                info = image.blob_info(blob)
                if info["kind"] != image.KIND_MFA or info["n_nodes"] > MAX_NODES or info["n_edges"] > MAX_EDGES:
                    continue
                out.append((regex, flag, blob, strings))
    return out


# ---- the GPU tests' fixed corpus -------------------------------------------------------------------------------------------------------
GPU_SEED, GPU_REGEXES, GPU_NCELL, GPU_SAMPLES = 0, 90, 9, 100
GPU_BATCH, GPU_BATCH_BYTES = 330, 900 * 1024

_gpu = None


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
        rng = random.Random(len(regex) + 31 * len(strings))
        batch, total = [], 0
        for s in strings:
            if len(batch) < GPU_BATCH and total + len(s) <= GPU_BATCH_BYTES:
                batch.append(s)
                total += len(s)
        if len(batch) < GPU_BATCH // 2:                     # (a regex of few distinct strings: the mixed batches need 131 of an image)
            continue
        if len(batch) % 64 == 0:
            batch.pop()
        rng.shuffle(batch)
        got[kind].append({"regex": regex, "flag": flag, "blob": blob, "cells": info["n_cells"], "edges": info["n_edges"], "strings": batch})
    for k in want:
        assert len(got[k]) == want[k], "the corpus holds %d %s images, %d wanted" % (len(got[k]), k, want[k])
    _gpu = got["few"] + got["mid"] + got["wide"] + got["bnf"] + got["rev"]
    return _gpu


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
