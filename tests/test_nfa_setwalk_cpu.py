"""The set walk of memory-less automata whose tabulation passes the limit, the part that can be wrong without a GPU (csrc/nfa_set_core.h:
the reference's step on a bit mask of live nodes, the walk of one string; csrc/image_host.cpp: the tables, the fall-over at image
creation), compiled for the host (tests/emul/nfa_set_emul.cpp) and run against the tabulated step function and the CPU restatement; and
what the C-ABI answers before it touches a device.  The kernel around it is checked by tests/test_nfa_setwalk_gpu.py, on the same
corpus (tests/testlib.py: setwalk_corpus)."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

import oracle_lib
from mfa_amd import capi, image
from testlib import (DIPLOMA, LENGTHS, NFA_NAMES, blob_of, emul_exe, expected, front_end_blob, k_regex, out_offsets, rand_regex, setwalk_corpus, table_127, wide_images,
                     wide_strings, write_batch)


@pytest.fixture(scope="module")
def emul():
    return emul_exe("nfa_set")


def run_match(emul, tmp_path, blob, strings):
    (tmp_path / "a.blob").write_bytes(blob)
    write_batch(tmp_path / "batch.bin", strings)
    p = subprocess.run([emul, "match", str(tmp_path / "a.blob"), str(tmp_path / "batch.bin")], capture_output=True)
    if p.returncode == 3:
        return None                                        # outside the set walk's limits (an epsilon cycle, too many nodes)
    assert p.returncode == 0, p.stderr.decode()[-400:]
    return np.frombuffer(p.stdout.strip(), dtype=np.uint8) - ord("0")


# ---- the step against the table: the proof for the restatement with masks -----------------------------------------------------------
EXTRA = {"k5_thompson": (k_regex(5), "-thompson"), "k5_glushkov": (k_regex(5), "-glushkov"),
         "k8_thompson": (k_regex(8), "-thompson"), "k8_glushkov": (k_regex(8), "-glushkov")}


@pytest.mark.parametrize("name", NFA_NAMES + sorted(EXTRA) + ["table_127"])
def test_step_equals_the_table(emul, name, tmp_path):
    """from EVERY tabulated state set and for EVERY byte class the core's step on the node mask reaches the set the table's row names, and
    accepts when the table does"""
    if name in EXTRA:
        blob = front_end_blob(EXTRA[name][0], tmp_path, 0, EXTRA[name][1])
    else:
        blob = table_127(tmp_path) if name == "table_127" else blob_of(name, 0)
    (tmp_path / "a.blob").write_bytes(blob)
    p = subprocess.run([emul, "step", str(tmp_path / "a.blob")], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()[-400:]
    f = p.stdout.split()
    info = capi.Image(blob).info()
    assert f[0] == b"ok" and (int(f[1]), int(f[2])) == (info["dfa_states"], info["byte_classes"])
    assert int(f[3]) == (1 if info["n_nodes"] <= 32 else 2 if info["n_nodes"] <= 64 else 4 if info["n_nodes"] <= 128 else 8)
    if name == "table_127":
        assert int(f[1]) == 127
    if name == "k8_thompson":
        assert int(f[1]) == 2 ** 9 + 2 and int(f[3]) == 2 and int(f[4]) >= 2      # two mask words, a stack in use


# ---- whole strings against the oracle -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rev", [0, 1], ids=["forward", "reversed"])
@pytest.mark.parametrize("name", NFA_NAMES)
def test_strings_against_oracle(emul, name, rev, tmp_path):
    blob, strings, golden = setwalk_corpus(name, rev)
    assert {o % 16 for o in out_offsets(strings)} == set(range(16)) and set(LENGTHS) <= {len(s) for s in strings}
    assert image.blob_info(blob)["reversed"] >= rev
    want = expected(blob, strings, golden)
    got = run_match(emul, tmp_path, blob, strings)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s: %d mismatches, first len %d want %d" % (name, bad.size, len(strings[bad[0]]), want[bad[0]])


def test_wider_masks_and_deep_chains(emul, tmp_path):
    rng = np.random.default_rng(77)
    seen_w = set()
    for key, blob in wide_images(tmp_path).items():
        strings = wide_strings(rng)
        want = oracle_lib.OracleImage(blob).match(strings)
        assert 0 < int(want.sum()) < len(strings), key
        got = run_match(emul, tmp_path, blob, strings)
        assert got is not None and np.array_equal(got, want), key
        n = image.blob_info(blob)["n_nodes"]
        seen_w.add(1 if n <= 32 else 2 if n <= 64 else 4 if n <= 128 else 8)
    assert {2, 4, 8} <= seen_w


@pytest.mark.parametrize("seed", range(4))
def test_front_end_fuzz(emul, seed, tmp_path):
    """random regexes without backreferences through the host front-end, every compile, forced to the set walk, against the oracle"""
    rng = random.Random(3000 + seed)
    nrng = np.random.default_rng(seed)
    checked = both = 0
    for _ in range(30):
        regex = rand_regex(rng, rng.randint(1, 3), [], False)
        if len(regex) < 2:
            continue
        for flag in ("-thompson", "-glushkov", ""):
            p = subprocess.run([DIPLOMA, "-dump"] + ([flag] if flag else []), input=regex + "\n", capture_output=True, text=True, cwd=tmp_path)
            assert p.returncode == 0, (regex, flag, p.stderr)
            blob = image.blob_from_dump(p.stdout)
            if image.blob_info(blob)["kind"] != image.KIND_NFA:
                continue
            strings = [bytes(nrng.choice(list(b"aabbc."), size=int(ln)).tolist()) for ln in nrng.integers(0, 24, size=150)]
            got = run_match(emul, tmp_path, blob, strings)
            if got is None:
                continue                                    # an epsilon cycle: refused at image creation (the reference would not return)
            want = oracle_lib.OracleImage(blob).match(strings)
            assert np.array_equal(got, want), "regex %r %s" % (regex, flag)
            checked += 1
            both += 0 < int(want.sum()) < len(strings)
    assert checked > 40 and both > 15


# ---- image creation and the C-ABI, before a device is touched -----------------------------------------------------------------------
@pytest.fixture()
def env(monkeypatch):
    for k in ("MFA_NFA_SETWALK", "MFA_DFA_STATE_LIMIT"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def k20_blob(tmp_path):
    return front_end_blob(k_regex(20), tmp_path, 0, "-thompson")


def test_k20_becomes_a_set_walk_image(env, tmp_path):
    """2^21 state sets: refused until now (MFA_ERR_UNSUPPORTED), a set-walk image from now on; it hands no state from call to call"""
    img = capi.Image(k20_blob(tmp_path))
    info = img.info()
    assert (info["kind"], info["dfa_states"], info["byte_classes"], info["last_kernel"]) == (image.KIND_NFA, 0, 3, capi.KERNEL_NONE)
    assert info["n_nodes"] > 64
    buf, off, res = (ctypes.c_uint8 * 64)(), (ctypes.c_uint64 * 2)(0, 3), (ctypes.c_uint8 * 4)()
    st = (ctypes.c_uint32 * 4)(1, 1, 1, 1)
    L = capi.lib()
    assert L.mfa_match_batch_resume(img._h, buf, off, 1, st, res, 0, None) == capi.ERR_UNSUPPORTED
    assert L.mfa_match_batch_resume_host(img._h, buf, off, 1, st, res, 0) == capi.ERR_UNSUPPORTED
    assert list(st) == [1, 1, 1, 1]


def test_setwalk_0_refuses_as_before(env, tmp_path):
    """the old refusal, on the k = 10 image under a limit of 1000 state sets: tabulating the k = 20 image to 2^20 sets takes 2.4 s and
    several hundred MB, so the suite does that once (test_k20_becomes_a_set_walk_image) and the path behind the limit is the same"""
    env.setenv("MFA_NFA_SETWALK", "0")
    env.setenv("MFA_DFA_STATE_LIMIT", "1000")
    with pytest.raises(capi.MfaError) as e:
        capi.Image(front_end_blob(k_regex(10), tmp_path, 0, "-thompson"))
    assert e.value.code == capi.ERR_UNSUPPORTED


def test_state_limit_and_forced_set_walk(env, tmp_path):
    blob = front_end_blob(k_regex(10), tmp_path, 0, "-thompson")
    assert capi.Image(blob).info()["dfa_states"] == 2050
    env.setenv("MFA_DFA_STATE_LIMIT", "1000")
    assert capi.Image(blob).info()["dfa_states"] == 0
    env.setenv("MFA_NFA_SETWALK", "0")
    with pytest.raises(capi.MfaError):
        capi.Image(blob)
    env.delenv("MFA_DFA_STATE_LIMIT")
    env.setenv("MFA_NFA_SETWALK", "1")
    small = capi.Image(blob_of("nfa_abb_thompson", 0)).info()
    assert (small["dfa_states"], small["byte_classes"]) == (0, 3)
    env.delenv("MFA_NFA_SETWALK")
    assert capi.Image(blob_of("nfa_abb_thompson", 0)).info()["dfa_states"] == 6


def test_epsilon_cycle_is_refused(env):
    """start -eps-> 2 -eps-> 3 -eps-> 2: the reference's evaluateState would never return"""
    nodes = [{"rank": 0, "edges": [(None, 2, {})]}, {"rank": 1, "edges": []},
             {"rank": 2, "edges": [(b"a", 1, {}), (None, 3, {})]}, {"rank": 3, "edges": [(None, 2, {})]}]
    img = {"kind": image.KIND_NFA, "reversed": 0, "start": 0, "finish": 1, "nodes": nodes}
    for force in (None, "1"):
        if force:
            env.setenv("MFA_NFA_SETWALK", force)
        with pytest.raises(capi.MfaError) as e:
            capi.Image(image.to_blob(img))
        assert e.value.code == capi.ERR_UNSUPPORTED
    nodes[3]["edges"] = [(None, 1, {})]                       # the same graph without the cycle is an image
    assert capi.Image(image.to_blob(img)).info()["dfa_states"] == 0


def test_stream_and_match_blocks_refuse_a_set_walk_image(env, tmp_path):
    """Automata::Stream hands a state from block to block, which a set-walk image does not have: `diploma -match-blocks` says so and
    ends with status 1 before it touches a device; a tabulated image gets past that point (to the device, or to its absence)"""
    e = {k: v for k, v in os.environ.items() if k not in ("MFA_NFA_SETWALK", "MFA_DFA_STATE_LIMIT")}
    text = "(a|b)*abb\nababb\nexit\n"
    r = subprocess.run([DIPLOMA, "-match-blocks", "2"], input=text, capture_output=True, text=True, cwd=tmp_path, env=dict(e, MFA_NFA_SETWALK="1"))
    assert r.returncode == 1 and not any(ln in ("0", "1") for ln in r.stdout.split("\n"))      # (compile() prints its header; no answer line)
    assert r.stderr.startswith("diploma: Automata::Stream: the automaton's state sets pass the tabulation limit"), r.stderr
    r = subprocess.run([DIPLOMA, "-match-blocks", "2"], input=text, capture_output=True, text=True, cwd=tmp_path, env=e)
    assert "Automata::Stream" not in r.stderr and (r.returncode == 0 or "no usable HIP device" in r.stderr), r.stderr


def test_constant_equals_the_header():
    hdr = open(os.path.join(oracle_lib.ROOT, "include", "mfa_hip.h")).read()
    got = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+MFA_KERNEL_(\w+)\s+(\d+)u", hdr)}
    assert got == {"NONE": capi.KERNEL_NONE, "WALK": capi.KERNEL_WALK, "SPECIALISED": capi.KERNEL_SPECIALISED, "TABLE": capi.KERNEL_TABLE,
                   "NODESET": capi.KERNEL_NODESET} and capi.KERNEL_NODESET == 4
