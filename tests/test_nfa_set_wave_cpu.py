"""The wave-cooperative set walk of memory-less automata (one string per wave, the node set across the lanes: up to 2048 nodes), the part
that can be wrong without a GPU -- csrc/nfa_set_wave_core.h: the reference's step on a mask that lies across 64 lanes, the walk of one
string through rounds of 64 blocks; csrc/image_host.cpp: the wave tables and which image gets them -- compiled for the host
(tests/emul/nfa_set_wave_emul.cpp with the 64-lane primitives of tests/emul/wave_lanes.h) and run against the tabulated step function
and the CPU restatement; and what the C-ABI answers before it touches a device.  The kernel around it is checked by
tests/test_nfa_set_wave_gpu.py, on the same images and strings (tests/setwalk_lib.py)."""
import ctypes
import random
import subprocess

import numpy as np
import pytest

import nfa_fuzz
import oracle_lib
from mfa_amd import capi, image
from setwalk_lib import (COUNTER300, EDGE_LENGTHS, LANE_MAX_NODES, RAW_NODES, WAVE_MAX_NODES, eps_chain, raw_corpus_once, regex_strings, run_match, run_step,
                         wide_regex_images, words_of)
from testlib import DIPLOMA, LENGTHS, NFA_NAMES, blob_of, emul_exe, front_end_blob, k_regex, out_offsets, table_127

WORDS = capi.SET_STATE_WORDS


@pytest.fixture(scope="module")
def emul():
    return emul_exe("nfa_set_wave")


@pytest.fixture()
def env(monkeypatch):
    for k in ("MFA_NFA_SETWALK", "MFA_DFA_STATE_LIMIT", "MFA_SET_WAVE"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


# ---- image creation and the C-ABI, before a device is touched -----------------------------------------------------------------------
def refused_without_a_touch(img):
    """every resume call answers MFA_ERR_UNSUPPORTED on the image and leaves records, state words and results as they came"""
    L = capi.lib()
    buf, off = (ctypes.c_uint8 * 64)(), (ctypes.c_uint64 * 2)(0, 3)
    res = (ctypes.c_uint8 * 4)(7, 7, 7, 7)
    st = (ctypes.c_uint32 * (WORDS + 8))(*([0x5a5a5a5a] * (WORDS + 8)))
    at = ctypes.addressof(st)
    at += -at % 16                                                                  # a 16-byte aligned record inside st
    assert L.mfa_match_batch_resume_set(img._h, buf, off, 1, at, res, 0, None) == capi.ERR_UNSUPPORTED
    assert L.mfa_match_batch_resume_set_host(img._h, buf, off, 1, at, res, 0) == capi.ERR_UNSUPPORTED
    assert L.mfa_match_batch_resume_set(img._h, buf, off, 0, at, res, 0, None) == capi.ERR_UNSUPPORTED      # (refused before n is looked at)
    words = (ctypes.c_uint32 * 4)(1, 1, 1, 1)
    assert L.mfa_match_batch_resume(img._h, buf, off, 1, words, res, 0, None) == capi.ERR_UNSUPPORTED
    assert L.mfa_match_batch_resume_host(img._h, buf, off, 1, words, res, 0) == capi.ERR_UNSUPPORTED
    assert list(st) == [0x5a5a5a5a] * (WORDS + 8) and list(words) == [1, 1, 1, 1] and list(res) == [7, 7, 7, 7]
    assert img.info()["last_kernel"] == capi.KERNEL_NONE


def test_an_image_beyond_256_nodes_is_created(env, tmp_path):
    """(a^300)*, 303 nodes: MFA_ERR_UNSUPPORTED until now, a set-walk image from now on; it hands nothing from call to call"""
    blob = front_end_blob(COUNTER300, tmp_path)
    n_nodes = image.blob_info(blob)["n_nodes"]
    assert n_nodes > LANE_MAX_NODES
    env.setenv("MFA_NFA_SETWALK", "1")
    img = capi.Image(blob)
    info = img.info()
    assert (info["kind"], info["dfa_states"], info["n_nodes"], info["last_kernel"]) == (image.KIND_NFA, 0, n_nodes, capi.KERNEL_NONE)
    refused_without_a_touch(img)
    # ... and by the limit on state sets alone, as a caller meets it (the counter tabulates to about 300 sets)
    env.delenv("MFA_NFA_SETWALK")
    assert capi.Image(blob).info()["dfa_states"] > 100
    env.setenv("MFA_DFA_STATE_LIMIT", "100")
    assert capi.Image(blob).info()["dfa_states"] == 0
    env.setenv("MFA_NFA_SETWALK", "0")
    with pytest.raises(capi.MfaError) as e:                     # no set walk: the refusal of old
        capi.Image(blob)
    assert e.value.code == capi.ERR_UNSUPPORTED


def test_forced_wave_tables_on_a_narrow_image(env):
    """MFA_SET_WAVE=1 gives a narrow set-walk image wave tables: the resume calls refuse it; without the knob the same image is the lane
    kernel's and mfa_match_batch_resume_set takes it (n == 0: MFA_OK before a device is looked for).  The knob makes no set-walk image
    of one that tabulates."""
    blob = blob_of("nfa_abb_thompson", 0)
    L = capi.lib()
    st = (ctypes.c_uint32 * (WORDS + 8))()
    at = ctypes.addressof(st)
    at += -at % 16
    buf, off, res = (ctypes.c_uint8 * 64)(), (ctypes.c_uint64 * 2)(0, 3), (ctypes.c_uint8 * 4)()
    env.setenv("MFA_SET_WAVE", "1")
    assert capi.Image(blob).info()["dfa_states"] == 6
    env.setenv("MFA_NFA_SETWALK", "1")
    forced = capi.Image(blob)
    assert forced.info()["dfa_states"] == 0
    refused_without_a_touch(forced)
    env.delenv("MFA_SET_WAVE")
    lane = capi.Image(blob)
    assert lane.info()["dfa_states"] == 0
    assert L.mfa_match_batch_resume_set(lane._h, buf, off, 0, at, res, 0, None) == capi.OK
    assert L.mfa_match_batch_resume_set_host(lane._h, buf, off, 0, at, res, 0) == capi.OK
    env.setenv("MFA_SET_WAVE", "0")                           # anything but 1 is "off"
    assert L.mfa_match_batch_resume_set(capi.Image(blob)._h, buf, off, 0, at, res, 0, None) == capi.OK


def test_node_limits(env):
    """2048 nodes is an image, 2049 is not; both only as node sets (MFA_NFA_SETWALK=1: nothing is tabulated)"""
    env.setenv("MFA_NFA_SETWALK", "1")
    rng = random.Random(11)
    img = capi.Image(image.to_blob(nfa_fuzz.random_image(rng, WAVE_MAX_NODES, 6)))
    assert (img.info()["n_nodes"], img.info()["dfa_states"]) == (WAVE_MAX_NODES, 0)
    for n in (WAVE_MAX_NODES + 1, 3000):
        with pytest.raises(capi.MfaError) as e:
            capi.Image(image.to_blob(nfa_fuzz.random_image(rng, n, 6)))
        assert e.value.code == capi.ERR_UNSUPPORTED
    # the first width beyond the lane kernel, and the last inside it
    assert capi.Image(image.to_blob(nfa_fuzz.random_image(rng, LANE_MAX_NODES + 1, 6))).info()["dfa_states"] == 0
    assert capi.Image(image.to_blob(nfa_fuzz.random_image(rng, LANE_MAX_NODES, 6))).info()["dfa_states"] == 0


def narrow_deep_blob(tmp_path):
    """229 nodes and an epsilon chain of 58: narrow enough for the lane kernel, too deep for its stack"""
    deep = "a"
    for _ in range(14):
        deep = "((" + deep + "|b)|c)"
    blob = front_end_blob("(" + deep + ")*" + deep, tmp_path)
    d = image.parse_dump(subprocess.run([DIPLOMA, "-dump", "-thompson"], input="(" + deep + ")*" + deep + "\n", capture_output=True, text=True, cwd=tmp_path).stdout)
    assert len(d["nodes"]) <= LANE_MAX_NODES and eps_chain(d) > 49
    return blob


def test_a_narrow_image_with_a_deep_chain_stays_refused(env, tmp_path):
    """up to 256 nodes an image is built exactly as before, whatever its chain: beyond 49 nodes it is refused (the fuzz suites count
    refusals and resume every accepted image); only the forced form takes it"""
    blob = narrow_deep_blob(tmp_path)
    env.setenv("MFA_NFA_SETWALK", "1")
    with pytest.raises(capi.MfaError) as e:
        capi.Image(blob)
    assert e.value.code == capi.ERR_UNSUPPORTED
    env.setenv("MFA_SET_WAVE", "1")
    assert capi.Image(blob).info()["dfa_states"] == 0


# ---- the step against the table: the proof for the restatement across lanes -----------------------------------------------------------
EXTRA = {"k5_thompson": (k_regex(5), "-thompson"), "k5_glushkov": (k_regex(5), "-glushkov"),
         "k8_thompson": (k_regex(8), "-thompson"), "k8_glushkov": (k_regex(8), "-glushkov"), "counter_300": (COUNTER300, "-thompson")}


@pytest.mark.parametrize("name", NFA_NAMES + sorted(EXTRA) + ["table_127"])
def test_step_equals_the_table(emul, name, tmp_path, env):
    """from EVERY tabulated state set and for EVERY byte class the wave step on the mask across the lanes reaches, bit for bit, the set
    the table's row names, and accepts when the table does -- on wave tables of narrow images (the forced form) and of the 303-node
    counter"""
    if name in EXTRA:
        blob = front_end_blob(EXTRA[name][0], tmp_path, 0, EXTRA[name][1])
    else:
        blob = table_127(tmp_path) if name == "table_127" else blob_of(name, 0)
    states, classes, W, depth = run_step(emul, tmp_path, blob)
    info = capi.Image(blob).info()
    assert (states, classes) == (info["dfa_states"], info["byte_classes"]) and W == words_of(info["n_nodes"])
    if name == "table_127":
        assert states == 127
    if name == "k8_thompson":
        assert states == 2 ** 9 + 2 and W == 2 and depth >= 2                      # two lanes in use, a stack in use
    if name == "counter_300":
        assert info["n_nodes"] > LANE_MAX_NODES and W == 10 and states >= 300


# ---- whole strings against the oracle, which has no node limit ------------------------------------------------------------------------
REGEX_IMAGES = ("k_512", "k_512_rev", "k_1024", "k_2048", "deep")
BANDS = {"k_512": (256, 512), "k_512_rev": (256, 512), "k_1024": (512, 1024), "k_2048": (1024, 2048), "deep": (256, 2048)}


@pytest.mark.parametrize("name", REGEX_IMAGES)
def test_wide_regex_images_against_oracle(emul, name, tmp_path):
    blob, alphabet, min_len = wide_regex_images(tmp_path)[name]
    info = image.blob_info(blob)
    assert BANDS[name][0] < info["n_nodes"] <= BANDS[name][1] and info["reversed"] == (1 if name in ("k_512_rev", "deep") else 0)
    strings = regex_strings(np.random.default_rng(len(name)), alphabet, min_len)
    assert {o % 16 for o in out_offsets(strings)} == set(range(16)) and set(LENGTHS + EDGE_LENGTHS) <= {len(s) for s in strings}
    want = oracle_lib.OracleImage(blob).match(strings)
    assert 0 < int(want.sum()) < len(strings), name
    got = run_match(emul, tmp_path, blob, strings)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s: %d mismatches, first len %d want %d" % (name, bad.size, len(strings[bad[0]]), want[bad[0]])


def test_raw_images_against_oracle(emul, tmp_path):
    """raw random images of 257 to 2048 nodes, `finish` anywhere, both scan directions, on strings drawn from the automaton"""
    corpus, dropped = raw_corpus_once()
    assert 10 * dropped <= len(corpus) + dropped and {image.blob_info(b)["n_nodes"] for _, b, _, _ in corpus} == set(RAW_NODES)
    assert {image.blob_info(b)["reversed"] for _, b, _, _ in corpus} == {0, 1}
    for name, blob, strings, want in corpus:
        assert 0 < int(want.sum()) < len(strings), name
        assert {o % 16 for o in out_offsets(strings)} == set(range(16)) and set(LENGTHS + EDGE_LENGTHS) <= {len(s) for s in strings}
        got = run_match(emul, tmp_path, blob, strings)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, "%s: %d mismatches, first len %d want %d" % (name, bad.size, len(strings[bad[0]]), want[bad[0]])


# ---- sanitizers ---------------------------------------------------------------------------------------------------------------------------
def test_under_sanitizers(tmp_path):
    """the harness as a stand-alone program under ASan and UBSan: a wide image on the edge lengths (emul::read_batch gives the batch
    exactly the room the read rule makes readable, the stack exactly its slots, a mask row exactly its words), both scan directions,
    and the step of the 303-node counter"""
    exe = emul_exe("nfa_set_wave", "-fsanitize=address,undefined -fno-sanitize-recover=all")
    images = wide_regex_images(tmp_path)
    for name in ("k_512", "deep"):
        blob, alphabet, min_len = images[name]
        rng = np.random.default_rng(9)
        pick = lambda ln: bytes(rng.choice(list(alphabet), size=int(ln)).tolist())
        strings = [pick(ln) for ln in LENGTHS + EDGE_LENGTHS + [min_len + 5, 3, 1040, 7]]
        strings = strings + strings[::-1]                     # (the last string ends the buffer: its last block is the last readable one)
        want = oracle_lib.OracleImage(blob).match(strings)
        assert np.array_equal(run_match(exe, tmp_path, blob, strings), want), name
    name, blob, strings, want = raw_corpus_once()[0][-1]      # 2048 nodes: every lane and the last bit in use
    assert image.blob_info(blob)["n_nodes"] == WAVE_MAX_NODES
    assert np.array_equal(run_match(exe, tmp_path, blob, strings[:80]), want[:80])
    assert run_step(exe, tmp_path, front_end_blob(COUNTER300, tmp_path))[2] == 10
