"""What tests/test_search_cpu.py and tests/test_search_gpu.py share: the host harness tests/emul/search/search_emul.cpp (built here, with its own
compiler line), its output, the definition of a match inside a string on the oracle, the images and the batches --
TEST INFRASTRUCTURE ONLY: no tests, no fixtures, no marks in here."""
import atexit
import os
import shutil
import subprocess
import tempfile

import numpy as np

import oracle_lib
import testlib
from mfa_amd import image

_built = {}


def search_exe(flags=""):
    """tests/emul/search/search_emul.cpp with the flags of build.sh's dfa_split row, `flags` behind the caller's EMUL_FLAGS; once per session, in a
    temporary directory of its own; the compiler is heard only when it fails.  (The harness lives in a folder of its own: every
    NAME_emul.cpp directly under tests/emul/ is build.sh's to build, and this one has its own compiler line.)"""
    if flags not in _built:
        folder = tempfile.mkdtemp(prefix="search_emul_")
        atexit.register(shutil.rmtree, folder, ignore_errors=True)
        exe = os.path.join(folder, "search_emul")
        emul_flags = (os.environ.get("EMUL_FLAGS", "") + " " + flags).split()
        cmd = ["g++", "-O1", "-g", "-std=c++17"] + emul_flags + ["-Wall", "-Ishim", "-I.", "-Wno-unknown-pragmas", "-Wno-unused-function", "-Wno-unused-variable",
               "-I" + testlib.CSRC, "-I" + os.path.join(oracle_lib.ROOT, "include"), "-o", exe, os.path.join("search", "search_emul.cpp"),
               os.path.join(testlib.CSRC, "image_host.cpp"), os.path.join(testlib.CSRC, "search_tables.cpp")]
        p = subprocess.run(cmd, cwd=testlib.EMUL_DIR, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert p.returncode == 0, "building search_emul failed:\n%s" % p.stdout
        _built[flags] = exe
    return _built[flags]


# ---- the harness ------------------------------------------------------------------------------------------------------------------------
def emul_run(exe, blob, strings, tmp_path, check=False):
    """(results[n], spans[2n + 1], span_results[2n]) of the harness for the batch `strings` packed back to back"""
    (tmp_path / "search_image.blob").write_bytes(blob)
    testlib.write_batch(tmp_path / "search_batch.bin", strings)
    p = subprocess.run([exe, "run", str(tmp_path / "search_image.blob"), str(tmp_path / "search_batch.bin")] + (["check"] if check else []),
                       capture_output=True)
    assert p.returncode == 0, "search_emul: exit %d\n%s" % (p.returncode, p.stderr.decode()[-800:])
    n = len(strings)
    assert len(p.stdout) == n + 8 * (2 * n + 1) + 2 * n
    return (np.frombuffer(p.stdout, dtype=np.uint8, count=n), np.frombuffer(p.stdout, dtype="<u8", count=2 * n + 1, offset=n),
            np.frombuffer(p.stdout, dtype=np.uint8, count=2 * n, offset=n + 8 * (2 * n + 1)))


def emul_info(exe, blob, tmp_path):
    """per pass (states, accept_from, start_accepts, enters_start, row0_dead); None: the search refuses the image"""
    (tmp_path / "search_image.blob").write_bytes(blob)
    p = subprocess.run([exe, "info", str(tmp_path / "search_image.blob")], capture_output=True, text=True)
    if p.returncode == 3:
        return None
    assert p.returncode == 0, p.stderr[-800:]
    return [tuple(int(x) for x in line.split()) for line in p.stdout.strip().split("\n")]


def emul_plan(exe, s1, s2, n, cus):
    p = subprocess.run([exe, "plan", str(s1), str(s2), str(n), str(cus)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    w = p.stdout.split()
    return dict(form=w[0], lds1=int(w[1]), lds2=int(w[2]), grid1=int(w[3]), grid2=int(w[4]), per_cu1=int(w[5]), per_cu2=int(w[6]), tile=int(w[7]))


# ---- the definition, on the oracle ------------------------------------------------------------------------------------------------------
def oracle_spans(blob, strings):
    """per string (found, i, j) relative to the string: the leftmost-longest pair among ALL its substrings that the oracle's whole-string
    match accepts -- every distinct substring is asked once"""
    subs = sorted({s[i:j] for s in strings for i in range(len(s) + 1) for j in range(i, len(s) + 1)})
    answers = dict(zip(subs, oracle_lib.OracleImage(blob).match(subs)))
    out = []
    for s in strings:
        hit = (0, 0, 0)
        for i in range(len(s) + 1):
            js = [j for j in range(i, len(s) + 1) if answers[s[i:j]]]
            if js:
                hit = (1, i, js[-1])
                break
        out.append(hit)
    return out


def expected_outputs(strings, found_spans):
    """what mfa_search_batch leaves for strings packed back to back from offset 0, given per string (found, i, j) relative to it"""
    n = len(strings)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in strings], dtype=np.uint64)
    res = np.zeros(n, dtype=np.uint8)
    spans = np.zeros(2 * n + 1, dtype=np.uint64)
    sres = np.zeros(2 * n, dtype=np.uint8)
    for k, (f, i, j) in enumerate(found_spans):
        res[k] = sres[2 * k] = f
        spans[2 * k] = off[k] + np.uint64(i if f else 0)
        spans[2 * k + 1] = off[k] + np.uint64(j if f else 0)
    spans[2 * n] = off[n]
    return res, spans, sres


# ---- images -----------------------------------------------------------------------------------------------------------------------------
def images(tmp_path):
    """name -> (blob, alphabet): every memory-less fixture in both directions, table_66 and table_127 in both, (a|b)^5 a"""
    out = {}
    for name in testlib.NFA_NAMES:
        alpha = b"abc" if name.startswith(("nfa_enum", "nfa_dot", "nfa_alt3", "nfa_star4")) else b"ab"
        for rev in (0, 1):
            out["%s_%s" % (name, "rev" if rev else "fwd")] = (testlib.fixture_blob(name, rev), alpha)
    for rev in (0, 1):
        out["table_66_%s" % ("rev" if rev else "fwd")] = (testlib.table_66(tmp_path, rev), b"ab")
        out["table_127_%s" % ("rev" if rev else "fwd")] = (testlib.table_127(tmp_path, rev), b"abcd")
    out["ab5a_fwd"] = (testlib.front_end_blob("(a|b)" * 5 + "a", tmp_path), b"ab")
    return out


def short_strings(name, alpha, rng, count=300):
    """`count` strings of 0 to 14 bytes over the image's letters plus z (table_127: over abcd alone, up to 16 bytes, so that matches occur)"""
    top, letters = (16, alpha) if name.startswith("table_127") else (14, alpha + b"z")
    out = [b"", alpha[:1], b"z"]
    while len(out) < count:
        ln = int(rng.integers(0, top + 1))
        s = testlib.rnd(letters, ln, rng)
        if name.startswith("table_127") and len(out) % 2:      # a(a|b)^5(c|d)^7 somewhere in every other string
            core = b"a" + testlib.rnd(b"ab", 5, rng) + testlib.rnd(b"cd", 7, rng)
            at = int(rng.integers(0, top - len(core) + 1))
            s = (testlib.rnd(letters, at, rng) + core + testlib.rnd(letters, top, rng))[:top]
            if name.endswith("_rev"):                          # the same automaton scanning from the end: the mirrored language
                s = s[::-1]
        out.append(s)
    return out


def long_strings(name, alpha, rng, count=120):
    """strings of 0 to 4097 bytes, packed back to back so that lines start at every offset mod 16: a few long ones (the brute force is
    quadratic), many short ones; matches near the begin, near the end and nowhere (a stretch of z cuts a line's matches short)"""
    letters = alpha
    lens =[0, 1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 255, 256, 257, 4095, 4096, 4097, 1000, 2049]
    lens += [int(x) for x in rng.integers(0, 300, size=count - len(lens))]
    out = []
    k = 0
    while lens or len({o % 16 for o in testlib.out_offsets(out)}) < 16:
        ln = lens.pop(0) if lens else int(rng.integers(1, 40))
        s = testlib.rnd(letters, ln, rng)
        if k % 4 == 1 and ln:
            s = b"z" * (ln - min(ln, 9)) + s[:min(ln, 9)]      # letters in the last nine bytes only
        elif k % 4 == 2 and ln:
            s = s[:min(ln, 9)] + b"z" * (ln - min(ln, 9))      # in the first nine only
        elif k % 4 == 3 and ln > 20:
            cut = int(rng.integers(0, ln))
            s = s[:cut] + b"z" + s[cut + 1:]
        elif k % 8 == 4:
            s = b"z" * ln                                      # nothing, unless the language holds the empty string
        out.append(s)
        k += 1
    return out


def info_reversed(blob):
    return image.blob_info(blob)["reversed"]
