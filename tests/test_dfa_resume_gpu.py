"""Memory-less automata on strings given in pieces, on the GPU: mfa_match_batch_resume (the resume instantiations of csrc/kernels.hip, and the fold of
csrc/dfa_split.hip started from a given state) against the CPU restatement and against the plain batch call, on the corpus of
tests/test_dfa_resume_cpu.py (tests/testlib.py); every table form; strings beyond MFA_MAX_STRING_BYTES; the sticky error; streams and capture; the host
mirror and the command line on top of it."""
import subprocess

import numpy as np
import pytest

import oracle_lib
from mfa_amd import capi, image
from testlib import (DEAD, DIPLOMA, INVALID, MAX_BYTES, NFA_NAMES, ROUNDS, START, accepted_long, blob_of, corpus, cuts_for, feed, filled, front_end_blob,
                     manifest_entry, match_on_gpu, new_states, pieces_against_whole, rnd, rounds_of, scan_poke, seen_so_far, states_of, table_66, table_127, upload)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("rev", [0, 1], ids=["forward", "reversed"])
@pytest.mark.parametrize("name", NFA_NAMES)
def test_piecewise_parity(name, rev):
    blob, strings, _ = corpus(name, rev)
    pieces_against_whole(capi.Image(blob), blob, strings, np.random.default_rng(len(name) * 977 + rev), "%s rev %d" % (name, rev))


@pytest.mark.parametrize("rev", [0, 1], ids=["forward", "reversed"])
@pytest.mark.parametrize("form", ["packed", "simple", "lds66", "lds127", "l2_514", "l2_32770", "l2_131074"])
def test_every_table_form(form, rev, tmp_path, monkeypatch):
    """an automaton mfa_match_batch would walk from SGPRs (the resume call takes the LDS table for it), the untiled LDS kernel on a small
    table, LDS-only tables of 66 and 127 state sets, and the L2 tables of 514, 32 770 (16-bit entries) and 131 074 (32-bit) state sets"""
    rng = np.random.default_rng(len(form) + 10 * rev)
    if form in ("packed", "simple"):
        monkeypatch.setenv("MFA_DFA_KERNEL", form)
        blob, strings, _ = corpus("nfa_abb_thompson", rev)
        states = None
    elif form.startswith("lds"):
        states = int(form[3:])
        blob = table_66(tmp_path, rev) if states == 66 else table_127(tmp_path, rev)
        alpha = b"ab" if states == 66 else b"aabbcd"
        strings = [rnd(alpha, int(ln), rng) for ln in [0, 1, 15, 16, 17, 4096, 20000] + [int(x) for x in rng.integers(0, 3000, size=150)]]
        strings += [rnd(b"ab", 900, rng) + t for t in (b"abbbbbcdcdcdcccc", b"abbbbb", b"babbbacdcdcdc", b"bbbbbb")]
    else:
        states = int(form.split("_")[1])
        k = {514: 8, 32770: 14, 131074: 16}[states]
        blob = front_end_blob("(a|b)*a" + "(a|b)" * k, tmp_path, rev)
        strings = [rnd(b"ab", int(ln), rng) for ln in rng.integers(0, 400, size=300)]
        strings += [b"", b"a" + b"b" * k, b"b" * (k + 1), b"ab" * 300 + b"a" + b"b" * k, b"ab" * 300 + b"b" + b"a" * k, b"abc" + b"a" * 30]
    if rev and states is not None:
        strings = [s[::-1] for s in strings]
    img = capi.Image(blob)
    assert states is None or img.info()["dfa_states"] == states
    pieces_against_whole(img, blob, strings, rng, form)
    want = oracle_lib.OracleImage(blob).match(strings)
    assert 0 < want.sum() < len(strings)


@pytest.mark.parametrize("rev", [0, 1], ids=["forward", "reversed"])
def test_table_between_lds_and_l2(rev, tmp_path):
    """130 state sets, a fused table of 67 080 bytes: beyond the 64 KiB of mfa_match_batch's LDS kernels (which refuses such an image, as it
    always has) and below the L2 kernel's 255 -- the resume call walks it with the untiled kernel, one workgroup per CU.  Pieces against
    the oracle on the whole strings and against one resume call on the whole strings."""
    k = 6
    blob = front_end_blob("(a|b)*a" + "(a|b)" * k, tmp_path, rev)
    rng = np.random.default_rng(130 + rev)
    strings = [rnd(b"ab", int(ln), rng) for ln in [0, 1, 15, 16, 17, 4096] + [int(x) for x in rng.integers(0, 1500, size=600)]]
    strings += [b"a" + b"b" * k, b"b" * (k + 1), b"ab" * 300 + b"a" + b"b" * k, b"ab" * 300 + b"b" + b"a" * k, b"abc" + b"a" * 30]
    if rev:
        strings = [s[::-1] for s in strings]
    n = len(strings)
    img = capi.Image(blob)
    assert img.info()["dfa_states"] == 130
    rounds = rounds_of(strings, cuts_for(strings, rng), rev)
    d_states = new_states(n)
    for r in range(ROUNDS):
        got = feed(img, [s[b:e] for s, (b, e) in zip(strings, rounds[r])], d_states)
    want = oracle_lib.OracleImage(blob).match(strings)
    assert 0 < want.sum() < n and np.array_equal(got, want)
    d_whole = new_states(n)
    assert np.array_equal(feed(img, strings, d_whole), want) and np.array_equal(states_of(d_states, n), states_of(d_whole, n))
    with pytest.raises(capi.MfaError) as err:
        match_on_gpu(img, strings)
    assert err.value.code == capi.ERR_UNSUPPORTED


LONG = (40 << 20) + 12345


def long_strings(which, rev, rng):
    """about 40 MiB each: accepted, rejected by the last byte scanned only, dead within the first few bytes scanned"""
    body = rnd(b"ab", LONG, rng)
    tail = {"abb": b"abb", "66": b"abbbbb", "127": b"abbbbb" + b"cdcdcdc" + b"ccc"}[which]
    ok = body[:LONG - len(tail)] + tail
    if rev:
        ok = ok[::-1]
    return [ok, scan_poke(ok, -1, rev), scan_poke(ok, 5, rev)]


@pytest.mark.parametrize("rev", [0, 1], ids=["forward", "reversed"])
@pytest.mark.parametrize("which", ["abb", "66", "127"])
def test_beyond_the_old_limit(which, rev, tmp_path):
    """strings of about 40 MiB as pieces of MFA_MAX_STRING_BYTES and a ragged rest: the answers are the oracle's on the WHOLE strings, and
    every call cuts its long pieces across the GPU (mfa_last_dfa_split), none is walked by one lane"""
    import torch
    blob = {"abb": lambda: blob_of("nfa_abb_thompson", rev), "66": lambda: table_66(tmp_path, rev), "127": lambda: table_127(tmp_path, rev)}[which]()
    strings = long_strings(which, rev, np.random.default_rng(len(which) + rev))
    want = oracle_lib.OracleImage(blob).match(strings)
    assert list(want) == [1, 0, 0]
    img = capi.Image(blob)
    d_states = new_states(len(strings))
    n_rounds = (LONG + MAX_BYTES - 1) // MAX_BYTES
    assert n_rounds == 3 and LONG > 2 * MAX_BYTES
    for r in range(n_rounds):
        if rev:
            pieces = [s[max(len(s) - (r + 1) * MAX_BYTES, 0):len(s) - r * MAX_BYTES] for s in strings]
        else:
            pieces = [s[r * MAX_BYTES:(r + 1) * MAX_BYTES] for s in strings]
        got = feed(img, pieces, d_states, results=(r == n_rounds - 1))
        n_cut = img.last_dfa_split()[0]
        assert n_cut == (3 if r == 0 else 2), (r, n_cut)       # the string that died in its first piece enters the later rounds dead
        st = states_of(d_states, 3)
        assert st[2] == DEAD and st[0] not in (DEAD, INVALID)
    assert list(got) == list(want)
    del strings, pieces
    torch.cuda.empty_cache()


def test_sticky_errors_and_dead_on_entry():
    """a word that names no state set (dfa_states itself), the error word, and a piece of limit + 1 bytes: result 2 and the error word, again
    after a following valid piece; a string that enters dead leaves dead with result 0; the neighbours in the batch are matched"""
    import torch
    blob = blob_of("nfa_abb_thompson", 0)
    img = capi.Image(blob)
    n_states = img.info()["dfa_states"]
    big = torch.full((MAX_BYTES + 1 + 64 + 16,), ord("a"), dtype=torch.uint8, device="cuda")
    big[:8] = torch.tensor(list(b"aabbaabb"), dtype=torch.uint8)
    big[8 + MAX_BYTES + 1:8 + MAX_BYTES + 1 + 8] = torch.tensor(list(b"abbaaabb"), dtype=torch.uint8)
    # strings: [0,4) aabb | [4,8) aabb | [8, 8 + limit + 1) too long | then abb, aa, abb (3, 2 and 3 bytes)
    e = 8 + MAX_BYTES + 1
    off = torch.tensor([0, 4, 8, e, e + 3, e + 5, e + 8], dtype=torch.int64, device="cuda")
    st_in = np.array([n_states, INVALID, START, START, DEAD, START], dtype=np.uint32)
    d_states = torch.from_numpy(st_in.view(np.int32)).cuda()
    res = filled(6)
    img.match_tensors_resume(big, off, d_states, res)
    torch.cuda.synchronize()
    st = states_of(d_states, 6)
    assert list(res.cpu().numpy()) == [2, 2, 2, 1, 0, 1] and list(st[:3]) == [INVALID] * 3 and st[4] == DEAD
    assert st[3] == st[5] and st[3] not in (DEAD, INVALID)
    # a valid piece for every string: the errors stay, the dead stays, the others go on ("abb" + "abb" is accepted, + "ab" is not)
    got = feed(img, [b"abb", b"abb", b"abb", b"abb", b"abb", b"ab"], d_states)
    st = states_of(d_states, 6)
    assert list(got) == [2, 2, 2, 1, 0, 0] and list(st[:3]) == [INVALID] * 3 and st[4] == DEAD and st[5] not in (DEAD, INVALID)
    # exactly the limit is a piece like any other (16 MiB - 1 of a and b, then abb: accepted)
    d_one = new_states(1)
    img.match_tensors_resume(big[16:], torch.tensor([0, MAX_BYTES], dtype=torch.int64, device="cuda"), d_one, None)
    assert list(feed(img, [b"abb"], d_one)) == [1]


def test_no_result_bytes_on_intermediate_rounds():
    """d_results == NULL until the last round: the answers are the last round's, on short pieces and on pieces the split path takes"""
    blob = blob_of("nfa_abb_glushkov", 0)
    rng = np.random.default_rng(5)
    strings = [rnd(b"ab", n, rng) + t for n, t in ((300000, b"abb"), (10, b"abb"), (200001, b"ab"), (0, b""), (210000, b"abz"), (999, b"abb"))]
    img = capi.Image(blob)
    d_states = new_states(len(strings))
    thirds = [[s[k * len(s) // 3:(k + 1) * len(s) // 3] for s in strings] for k in range(3)]
    assert sum(len(t) >= 65536 for t in thirds[0]) == 3       # three first pieces of MFA_DFA_SPLIT_MIN bytes or more
    assert feed(img, thirds[0], d_states, results=False) is None and img.last_dfa_split()[0] == 3
    assert feed(img, thirds[1], d_states, results=False) is None
    got = feed(img, thirds[2], d_states)
    assert list(got) == list(oracle_lib.OracleImage(blob).match(strings)) and 0 < got.sum() < len(strings)


def test_two_streams_one_image():
    """one image, two streams, two batches of the same shape and different content in flight at once, three rounds each"""
    import torch
    blob = blob_of("nfa_abb_thompson", 0)
    rng = np.random.default_rng(77)
    lens = [300000, 50, 70001, 0, 1 << 20, 999, 65536, 65535]
    ora = oracle_lib.OracleImage(blob)
    img = capi.Image(blob)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    work = []
    for v in range(2):
        strings = [rnd(b"ab", ln, rng) for ln in lens]
        strings = [s[:-3] + b"abb" if (k + v) % 2 and len(s) >= 3 else s for k, s in enumerate(strings)]
        rounds = [upload([s[r * len(s) // 3:(r + 1) * len(s) // 3] for s in strings]) for r in range(3)]
        work.append((rounds, new_states(len(lens)), filled(len(lens)), ora.match(strings)))
    assert not np.array_equal(work[0][3], work[1][3])
    torch.cuda.synchronize()
    for r in range(3):
        for v in range(2):
            rounds, d_states, res, _ = work[v]
            img.match_tensors_resume(rounds[r][0], rounds[r][1], d_states, res if r == 2 else None, stream=streams[v])
    torch.cuda.synchronize()
    for rounds, d_states, res, want in work:
        assert np.array_equal(res.cpu().numpy(), want)


def test_resume_call_is_capturable():
    """as test_dfa_split_gpu.py::test_call_is_capturable: after a first uncaptured call, the call is captured on one stream (no parallel
    branches) and replayed with new states and new bytes in the same buffers"""
    import torch
    blob = blob_of("nfa_abb_glushkov", 0)
    rng = np.random.default_rng(12)
    first = [rnd(b"ab", 500000, rng), b"ab", rnd(b"ab", 900001, rng), b"abb", b""]
    second = [rnd(b"ab", len(s), rng) for s in first]
    second[0] = second[0][:-3] + b"abb"
    second[3] = b"bab"
    whole = [a + b for a, b in zip(first, second)]
    want_first, want_whole = oracle_lib.OracleImage(blob).match(first), oracle_lib.OracleImage(blob).match(whole)
    d_bytes, d_off, _ = upload(first)
    d_states = new_states(len(first))
    res = filled(len(first))
    img = capi.Image(blob)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        img.match_tensors_resume(d_bytes, d_off, d_states, res)       # allocates the workspace
    torch.cuda.synchronize()
    assert np.array_equal(res.cpu().numpy(), want_first) and img.last_dfa_split()[0] == 2
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        img.match_tensors_resume(d_bytes, d_off, d_states, res)
    torch.cuda.synchronize()
    for pieces, want in ((first, want_first), (second, want_whole)):  # replay 1: the first pieces again from START; replay 2: the second pieces on top
        if pieces is first:
            d_states.copy_(new_states(len(first)))
        data, _ = oracle_lib.pack(pieces)
        d_bytes[:len(data)] = torch.from_numpy(data.copy()).cuda()
        res.fill_(7)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(res.cpu().numpy(), want)


def test_host_entry_point():
    """mfa_match_batch_resume_host: two rounds with host pointers, no result bytes in the first"""
    blob = blob_of("nfa_abb_thompson", 0)
    strings = [b"ab" * 50 + b"abb", b"abb", b"", b"abz" * 9, b"b" * 70000 + b"abb"]
    img = capi.Image(blob)
    states = np.full(len(strings), START, dtype=np.uint32)
    d1, o1 = oracle_lib.pack([s[:len(s) // 2] for s in strings])
    d2, o2 = oracle_lib.pack([s[len(s) // 2:] for s in strings])
    assert img.match_host_resume(np.concatenate([d1, np.zeros(16, np.uint8)]), o1, states, want_results=False) is None
    got = img.match_host_resume(np.concatenate([d2, np.zeros(16, np.uint8)]), o2, states)
    assert list(got) == list(oracle_lib.OracleImage(blob).match(strings)) == [1, 1, 0, 0, 1]


# ---- the host mirror and the command line ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nfa_abb_plain", "nfa_alt3_plain"])
def test_cli_tokens_beyond_the_limit(name, tmp_path):
    """`diploma -match` with tokens of 20 MiB + 5 -- one accepted, one rejected by its last byte -- between two short ones: 0/1 lines as
    for any token, the header unchanged.  (a|b)*abb compiles to an automaton that scans from the END (the pieces go last first), the
    other regex to one that scans from the front.  `diploma -match-blocks` (an Automata::Stream fed 1 MiB at a time) agrees."""
    auto = manifest_entry(name)
    blob = blob_of(name, 0)
    assert image.blob_info(blob)["reversed"] == (1 if name == "nfa_abb_plain" else 0)
    rng = np.random.default_rng(20)
    n = (20 << 20) + 5
    ok = accepted_long(name, n, rng)
    tokens = [ok[:50] + ok[-50:], ok, ok[:-1] + b"A", ok[-20:]]
    assert len(ok) == n and n > MAX_BYTES
    want = oracle_lib.OracleImage(blob).match(tokens)
    assert list(want[1:3]) == [1, 0]
    text = auto["regex"].encode() + b"\n" + b"\n".join(tokens) + b"\nexit\n"
    p = subprocess.run([DIPLOMA, "-match"], input=text, capture_output=True, cwd=tmp_path)
    assert p.returncode == 0, p.stderr
    assert p.stdout == auto["header"].encode() + b"".join(b"%d\n" % w for w in want)
    p = subprocess.run([DIPLOMA, "-match-blocks", str(1 << 20)], input=text, capture_output=True, cwd=tmp_path)
    assert p.returncode == 0, p.stderr
    assert p.stdout == auto["header"].encode() + b"".join(b"%d\n" % w for w in want)


def test_cli_memory_regex_still_refuses_a_long_token(tmp_path):
    """a regex with memory: a token beyond the limit fails as it always has (MFA_ERR_TOO_LONG from the host entry point), a short one is matched"""
    auto = manifest_entry("ex1_plain")
    text = auto["regex"].encode() + b"\n" + b"aa\n" + b"a" * (MAX_BYTES + 1) + b"\nexit\n"
    p = subprocess.run([DIPLOMA, "-match"], input=text, capture_output=True, cwd=tmp_path)
    assert p.returncode != 0 and b"MFA_MAX_STRING_BYTES" in p.stderr
    p = subprocess.run([DIPLOMA, "-match-blocks", "4096"], input=auto["regex"].encode() + b"\naa\nexit\n", capture_output=True, cwd=tmp_path)
    assert p.returncode != 0 and b"memory" in p.stderr
