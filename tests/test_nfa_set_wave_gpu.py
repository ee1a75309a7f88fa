"""The wave-cooperative set walk of memory-less automata on the GPU (csrc/nfa_set_wave.hip: one string per wave, the node set across the
lanes): images of 257 to 2048 nodes against the CPU restatement, batch shapes that leave waves idle and that make the persistent loop
run, the forced form (MFA_SET_WAVE=1) on the narrow corpus against the oracle AND the lane kernel, a mixed object that holds a wide
image, the command line, and the refusal of strings in pieces.  Images and strings are those of tests/test_nfa_set_wave_cpu.py
(tests/setwalk_lib.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle_lib
from mfa_amd import capi, image
from setwalk_lib import COUNTER300, LANE_MAX_NODES, WAVE_MAX_NODES, raw_corpus_once, regex_strings, wide_regex_images
from testlib import DIPLOMA, NFA_NAMES, expected, filled, setwalk_corpus, upload

pytestmark = pytest.mark.gpu

GPU_RAW = (257, 1025, 2048)        # the first width beyond the lane engine, the first beyond half a wave, every lane and the last bit


@pytest.fixture()
def env(monkeypatch):
    for k in ("MFA_NFA_SETWALK", "MFA_DFA_STATE_LIMIT", "MFA_SET_WAVE", "MFA_SET_SPLIT"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def match_guarded(img, strings):
    """one mfa_match_batch call with exactly the room the read rule asks for behind the strings and 64 guard bytes on either side of the
    results: the strings' result bytes"""
    import torch
    n = len(strings)
    d_bytes, d_off, _ = upload(strings, exact=True)
    buf = torch.full((n + 128,), 7, dtype=torch.uint8, device="cuda")
    img.match_tensors(d_bytes, d_off, buf[64:64 + n])
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:64] == 7).all() and (host[64 + n:] == 7).all(), "a result byte outside the results"
    return host[64:64 + n].copy()


def check(img, strings, want, what):
    got = match_guarded(img, strings)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s: %d mismatches, first string %d (len %d) got %d want %d" % (what, bad.size, bad[0], len(strings[bad[0]]), got[bad[0]], want[bad[0]])
    assert img.info()["last_kernel"] == capi.KERNEL_NODESET
    assert img.last_set_split() == (0, 0, 0, 0, 0, 0) and img.last_dfa_split() == (0, 0, 0) and img.last_dfa_spec() == (0, 0, 0)
    assert img.last_kernel_ms() > 0.0


# ---- answers --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k_512", "k_512_rev", "k_1024", "k_2048", "deep"])
def test_wide_regex_images(env, name, tmp_path):
    """created with a low tabulation limit, so they fall over to the set walk by themselves -- and, beyond 256 nodes, to the wave kernel"""
    blob, alphabet, min_len = wide_regex_images(tmp_path)[name]
    strings = regex_strings(np.random.default_rng(len(name)), alphabet, min_len)
    want = oracle_lib.OracleImage(blob).match(strings)
    assert 0 < int(want.sum()) < len(strings)
    env.setenv("MFA_DFA_STATE_LIMIT", "2")                             # (the deep image has eight state sets)
    img = capi.Image(blob)
    assert img.info()["dfa_states"] == 0 and img.info()["n_nodes"] > LANE_MAX_NODES
    check(img, strings, want, name)


def test_raw_images(env):
    """raw random images of 257, 1025 and 2048 nodes, both scan directions, on strings drawn from the automaton"""
    corpus, dropped = raw_corpus_once(GPU_RAW, 2)
    assert dropped == 0 and {image.blob_info(b)["n_nodes"] for _, b, _, _ in corpus} == set(GPU_RAW)
    assert {image.blob_info(b)["reversed"] for _, b, _, _ in corpus} == {0, 1}
    env.setenv("MFA_NFA_SETWALK", "1")
    for name, blob, strings, want in corpus:
        check(capi.Image(blob), strings, want, name)


# ---- shapes ---------------------------------------------------------------------------------------------------------------------------
def test_batch_shapes(env):
    """1, 3, 4, 5 and 1027 strings: idle waves in a block, a count that is no multiple of 4; and 20 000 strings of at most 8 bytes on
    the 257-node image: more strings than resident waves (256 CUs x 32), so the persistent loop runs"""
    name, blob, strings, want = raw_corpus_once(GPU_RAW, 2)[0][0]
    info = image.blob_info(blob)
    assert info["n_nodes"] == 257 and info["reversed"] == 0
    env.setenv("MFA_NFA_SETWALK", "1")
    img = capi.Image(blob)
    acc, rej = np.nonzero(want == 1)[0], np.nonzero(want == 0)[0]
    order = [acc[0], rej[0], acc[1], rej[1], acc[2]] + list(range(len(strings)))      # both answers in the small batches
    for n in (1, 3, 4, 5, 1027):
        pick = [int(order[k % len(order)]) for k in range(n)]
        check(img, [strings[k] for k in pick], want[pick], "%s, %d strings" % (name, n))
    short = [strings[k % len(strings)][:(k // len(strings)) % 9] for k in range(20000)]      # prefixes: the image scans forward
    want_short = oracle_lib.OracleImage(blob).match(short)
    assert max(len(s) for s in short) <= 8 and len(short) > 256 * 32
    check(img, short, want_short, name + ", 20 000 short strings")


# ---- the forced form on the narrow corpus -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NFA_NAMES)
def test_forced_form_equals_the_lane_kernel(env, name):
    """MFA_SET_WAVE=1: every memory-less fixture, both directions, walked by the wave kernel: the oracle's answers, and byte for byte
    what the lane kernel gives without the knob on the same strings"""
    for rev in (0, 1):
        blob, strings, golden = setwalk_corpus(name, rev)
        want = expected(blob, strings, golden)
        env.setenv("MFA_NFA_SETWALK", "1")
        env.delenv("MFA_SET_WAVE", raising=False)
        lane = capi.Image(blob)
        env.setenv("MFA_SET_WAVE", "1")
        wave = capi.Image(blob)
        assert lane.info()["dfa_states"] == 0 and wave.info()["dfa_states"] == 0
        got_lane = match_guarded(lane, strings)
        check(wave, strings, want, "%s rev %d" % (name, rev))
        assert np.array_equal(match_guarded(wave, strings), got_lane)
        # the knob chose the kernel: the wave image hands nothing from call to call, the lane image does
        L = capi.lib()
        assert L.mfa_match_batch_resume_set(wave._h, None, (ctypes.c_uint64 * 1)(0), 0, 16, None, 0, None) == capi.ERR_UNSUPPORTED
        assert L.mfa_match_batch_resume_set(lane._h, None, (ctypes.c_uint64 * 1)(0), 0, 16, None, 0, None) == capi.OK


# ---- a mixed object ---------------------------------------------------------------------------------------------------------------------
def test_one_mixed_object(env, tmp_path):
    """a memory automaton, a tabulated image and a wide image in one object: the answers of the three per-image calls, the wide
    segment as a launch of its own"""
    import torch
    env.setenv("MFA_MIXED_DFA", "1")
    mem_blob = image.blob_from_dump(oracle_lib.load_dump("ex1_plain"))
    tab_blob = image.blob_from_dump(oracle_lib.load_dump("nfa_abb_thompson"))
    wide_blob, alphabet, min_len = wide_regex_images(tmp_path)["k_512"]
    mem, tab = capi.Image(mem_blob), capi.Image(tab_blob)
    env.setenv("MFA_DFA_STATE_LIMIT", "100")
    wide = capi.Image(wide_blob)
    env.delenv("MFA_DFA_STATE_LIMIT")
    assert (tab.info()["dfa_states"], wide.info()["dfa_states"]) == (6, 0) and wide.info()["n_nodes"] > LANE_MAX_NODES
    base = oracle_lib.load_set("abc7")[:700]
    seg_wide = regex_strings(np.random.default_rng(6), alphabet, min_len)
    segments = [base, base, seg_wide]
    strings = [s for seg in segments for s in seg]
    d_bytes, d_off, _ = upload(strings, exact=True)
    res = filled(len(strings))
    mixed = capi.Mixed([mem, tab, wide])
    mixed.match_tensors(d_bytes, d_off, [0, 700, 1400, 1400 + len(seg_wide)], res)
    torch.cuda.synchronize()
    got = res.cpu().numpy()
    each = [match_guarded(im, seg) for im, seg in zip((mem, tab, wide), segments)]
    want = np.concatenate([oracle_lib.OracleImage(b).match(seg) for b, seg in zip((mem_blob, tab_blob, wide_blob), segments)])
    assert np.array_equal(np.concatenate(each), want) and np.array_equal(got, want)
    assert all(0 < int(e.sum()) < len(e) for e in each)
    d = mixed.last_dfa()
    assert (d["multi_launches"], d["own_launches"], d["items"], d["strings"]) == (1, 1, 1, 700)
    assert wide.info()["last_kernel"] == capi.KERNEL_NODESET
    mixed.close()


# ---- the command line -------------------------------------------------------------------------------------------------------------------
def test_command_line(env, tmp_path):
    """`diploma -match` on (a^300)* under a limit of 100 state sets: more than 256 nodes, walked by the wave kernel; the oracle's answers
    (a line of the command line carries no empty string)"""
    words = ["a" * 300, "a" * 299, "a" * 600, "a", "a" * 301, "a" * 900, "a" * 150 + "b" + "a" * 149, "b"]
    p = subprocess.run([DIPLOMA, "-dump"], input=COUNTER300 + "\n", capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode == 0, p.stderr
    blob = image.blob_from_dump(p.stdout)
    assert image.blob_info(blob)["n_nodes"] > LANE_MAX_NODES
    want = oracle_lib.OracleImage(blob).match([w.encode() for w in words])
    assert [int(x) for x in want] == [1, 0, 1, 0, 0, 1, 0, 0]
    e = {k: v for k, v in os.environ.items() if k not in ("MFA_NFA_SETWALK", "MFA_SET_WAVE")}
    e.update(MFA_DFA_STATE_LIMIT="100", MFA_VERBOSE="1")
    r = subprocess.run([DIPLOMA, "-match"], input=COUNTER300 + "\n" + "\n".join(words) + "\nexit\n", capture_output=True, text=True, cwd=tmp_path, env=e)
    assert r.returncode == 0, r.stderr
    assert [int(x) for x in r.stdout.split() if x in ("0", "1")] == [int(x) for x in want]
    assert "nfa_set_wave_kernel" in r.stderr


# ---- strings in pieces are refused, with a device present ---------------------------------------------------------------------------------
def test_resume_set_is_refused_on_the_device(env):
    """mfa_match_batch_resume_set on a wave image: MFA_ERR_UNSUPPORTED; records, results and their guard bytes as they came"""
    import torch
    assert capi.device_count() > 0
    name, blob, strings, want = raw_corpus_once(GPU_RAW, 2)[0][-1]
    assert image.blob_info(blob)["n_nodes"] == WAVE_MAX_NODES
    env.setenv("MFA_NFA_SETWALK", "1")
    img = capi.Image(blob)
    check(img, strings[:40], want[:40], name)                      # the image is on the device
    n = 40
    d_bytes, d_off, _ = upload(strings[:n], exact=True)
    recs = torch.full((n * capi.SET_STATE_WORDS + 32,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    res = torch.full((n + 128,), 7, dtype=torch.uint8, device="cuda")
    at = recs.data_ptr() + 64
    assert at % 16 == 0
    rc = capi.lib().mfa_match_batch_resume_set(img._h, d_bytes.data_ptr(), d_off.data_ptr(), n, at, res.data_ptr() + 64, 0, None)
    torch.cuda.synchronize()
    assert rc == capi.ERR_UNSUPPORTED
    assert (recs.cpu().numpy() == 0x5a5a5a5a).all() and (res.cpu().numpy() == 7).all()
    states = np.full(n * capi.SET_STATE_WORDS, 0x5a5a5a5a, dtype=np.uint32)
    data, off = oracle_lib.pack(strings[:n])
    with pytest.raises(capi.MfaError) as e:
        img.match_host_resume_set(np.concatenate([data, np.zeros(16, np.uint8)]), off, states)
    assert e.value.code == capi.ERR_UNSUPPORTED and (states == 0x5a5a5a5a).all()
