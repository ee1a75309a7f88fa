"""The set walk of memory-less automata on the GPU (csrc/nfa_set.hip): every memory-less fixture forced onto it, the automatic fall-over
of an automaton with 2^21 state sets, wider masks and deep epsilon chains, a mixed object that holds one, and the command line -- against
the golden answers and the CPU restatement.  Corpus and images are those of tests/test_nfa_setwalk_cpu.py (tests/testlib.py)."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib
from mfa_amd import capi, image
from testlib import DIPLOMA, LENGTHS, NFA_NAMES, expected, filled, front_end_blob, k_regex, match_on_gpu, setwalk_corpus, upload, wide_images, wide_strings

pytestmark = pytest.mark.gpu


@pytest.fixture()
def env(monkeypatch):
    for k in ("MFA_NFA_SETWALK", "MFA_DFA_STATE_LIMIT"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def match(img, strings):
    """with exactly the room the read rule asks for behind the strings"""
    return match_on_gpu(img, strings, exact=True)[0]


def check(img, strings, want, what):
    got = match(img, strings)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s: %d mismatches, first string %d (len %d) got %d want %d" % (what, bad.size, bad[0], len(strings[bad[0]]), got[bad[0]], want[bad[0]])
    assert img.info()["last_kernel"] == capi.KERNEL_NODESET
    assert img.last_dfa_split() == (0, 0, 0) and img.last_dfa_spec() == (0, 0, 0) and img.last_kernel_ms() > 0.0


@pytest.mark.parametrize("rev", [0, 1], ids=["forward", "reversed"])
@pytest.mark.parametrize("name", NFA_NAMES)
def test_fixtures_forced(env, name, rev):
    """every memory-less fixture as a set-walk image, about 600 strings, against the reference's golden answers and the CPU restatement;
    the same image on fewer than 64 strings and on a count that is no multiple of 256"""
    blob, strings, golden = setwalk_corpus(name, rev)
    want = expected(blob, strings, golden)
    assert set(LENGTHS) <= {len(s) for s in strings} and len(strings) % 256 != 0 and len(strings) > 512
    env.setenv("MFA_NFA_SETWALK", "1")
    img = capi.Image(blob)
    assert img.info()["dfa_states"] == 0
    check(img, strings, want, name)
    few = list(range(len(strings) - 45, len(strings)))                # the generated tail: long and short, both answers
    if 0 < int(want[few].sum()) < len(few):
        check(img, [strings[k] for k in few], want[few], name + " (45 strings)")
    else:
        few = [int(k) for k in np.nonzero(want)[0][:20]] + [int(k) for k in np.nonzero(want == 0)[0][:25]]
        check(img, [strings[k] for k in few], want[few], name + " (45 strings)")


def test_automatic_fall_over(env, tmp_path):
    """(a|b)*a(a|b)^20: the Thompson compile has 2^21 state sets and falls over to the set walk by itself; the plain compile scans from
    the end, has 45 and stays tabulated.  Both against the oracle, the Thompson one on a string of 70 000 bytes too, walked whole"""
    rng = np.random.default_rng(20)
    rnd = lambda k: bytes(rng.choice(list(b"ab"), size=k).tolist())
    strings = [b"a" + b"b" * 20, b"b" + b"a" * 20, rnd(600) + b"a" + b"b" * 20, rnd(600) + b"b" + b"a" * 20, rnd(69979) + b"a" + rnd(20), b"", b"a", b"a" * 20, b"a" * 21]
    strings += [rnd(int(ln)) for ln in rng.integers(0, 300, size=300)] + [rnd(40) + b"c" + rnd(30)]
    assert len(strings[4]) == 70000
    thompson = front_end_blob(k_regex(20), tmp_path, 0, "-thompson")
    want = oracle_lib.OracleImage(thompson).match(strings)
    assert list(want[:5]) == [1, 0, 1, 0, 1] and 0 < int(want.sum()) < len(strings)
    img = capi.Image(thompson)
    assert img.info()["dfa_states"] == 0 and img.info()["n_nodes"] > 64
    check(img, strings, want, "thompson")
    p = subprocess.run([DIPLOMA, "-dump"], input=k_regex(20) + "\n", capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode == 0, p.stderr
    plain = image.blob_from_dump(p.stdout)
    want_plain = oracle_lib.OracleImage(plain).match(strings)
    assert np.array_equal(want_plain, want)                            # the same language
    pimg = capi.Image(plain)
    assert np.array_equal(match(pimg, strings), want)
    assert pimg.info()["last_kernel"] == (capi.KERNEL_NODESET if pimg.info()["dfa_states"] == 0 else capi.KERNEL_TABLE)
    env.setenv("MFA_NFA_SETWALK", "1")                                 # and the plain compile as a set-walk image: the reversed scan
    forced = capi.Image(plain)
    assert forced.info()["is_reversed"] == 1
    check(forced, strings, want, "plain, forced")


def test_wider_masks_and_deep_chains(env, tmp_path):
    """Thompson of nested alternations: two, four and eight mask words, and epsilon chains that need the stack; created with a low
    tabulation limit, so they fall over by themselves"""
    rng = np.random.default_rng(78)
    env.setenv("MFA_DFA_STATE_LIMIT", "2")                             # (the deep image has five state sets)
    for key, blob in wide_images(tmp_path).items():
        strings = wide_strings(rng, 600)
        want = oracle_lib.OracleImage(blob).match(strings)
        assert 0 < int(want.sum()) < len(strings), key
        img = capi.Image(blob)
        assert img.info()["dfa_states"] == 0, key
        check(img, strings, want, key)


def test_one_mixed_object(env, tmp_path):
    """a memory automaton, a tabulated image and a set-walk image in one object: the answers of the three per-image calls, the set-walk
    segment as a launch of its own"""
    import torch
    env.setenv("MFA_MIXED_DFA", "1")
    mem_blob = image.blob_from_dump(oracle_lib.load_dump("ex1_plain"))
    tab_blob = image.blob_from_dump(oracle_lib.load_dump("nfa_abb_thompson"))
    set_blob = front_end_blob(k_regex(10), tmp_path, 0, "-thompson")
    mem, tab = capi.Image(mem_blob), capi.Image(tab_blob)
    env.setenv("MFA_DFA_STATE_LIMIT", "1000")
    sw = capi.Image(set_blob)
    env.delenv("MFA_DFA_STATE_LIMIT")
    assert (tab.info()["dfa_states"], sw.info()["dfa_states"]) == (6, 0)
    rng = np.random.default_rng(5)
    base = oracle_lib.load_set("abc7")[:700]
    seg_set = [bytes(rng.choice(list(b"ab"), size=int(ln)).tolist()) for ln in rng.integers(0, 200, size=500)]
    segments = [base, base, seg_set]
    strings = [s for seg in segments for s in seg]
    d_bytes, d_off, _ = upload(strings, exact=True)
    res = filled(len(strings))
    mixed = capi.Mixed([mem, tab, sw])
    mixed.match_tensors(d_bytes, d_off, [0, 700, 1400, 1900], res)
    torch.cuda.synchronize()
    got = res.cpu().numpy()
    each = [match(im, seg) for im, seg in zip((mem, tab, sw), segments)]
    want = np.concatenate([oracle_lib.OracleImage(b).match(seg) for b, seg in zip((mem_blob, tab_blob, set_blob), segments)])
    assert np.array_equal(np.concatenate(each), want) and np.array_equal(got, want)
    assert all(0 < int(e.sum()) < len(e) for e in each)
    d = mixed.last_dfa()
    assert (d["multi_launches"], d["own_launches"], d["items"], d["strings"]) == (1, 1, 1, 700)
    assert sw.info()["last_kernel"] == capi.KERNEL_NODESET
    mixed.close()


def test_command_line(env, tmp_path):
    """`diploma -match` on the k = 20 regex, as it compiles it and with every memory-less image forced to the set walk"""
    rng = np.random.default_rng(9)
    words = ["a" + "b" * 20, "b" + "a" * 20, "ab" * 40] + ["".join(rng.choice(list("ab"), size=int(ln)).tolist()) for ln in rng.integers(1, 120, size=60)]
    p = subprocess.run([DIPLOMA, "-dump"], input=k_regex(20) + "\n", capture_output=True, text=True, cwd=tmp_path)
    want = oracle_lib.OracleImage(image.blob_from_dump(p.stdout)).match([w.encode() for w in words])
    assert 0 < int(want.sum()) < len(words)
    for force in (None, "1"):
        e = dict(os.environ)
        e.pop("MFA_NFA_SETWALK", None)
        if force:
            e["MFA_NFA_SETWALK"] = force
            e["MFA_VERBOSE"] = "1"
        r = subprocess.run([DIPLOMA, "-match"], input=k_regex(20) + "\n" + "\n".join(words) + "\nexit\n", capture_output=True, text=True, cwd=tmp_path, env=e)
        assert r.returncode == 0, r.stderr
        got = [int(x) for x in r.stdout.split() if x in ("0", "1")]
        assert got == [int(x) for x in want], force
        if force:
            assert "nfa_set_kernel" in r.stderr
