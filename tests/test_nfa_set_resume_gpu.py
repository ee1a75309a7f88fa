"""Set-walk images on strings given in pieces, on the GPU: mfa_match_batch_resume_set (nfa_set_resume_kernel, csrc/nfa_set.hip) against the CPU
restatement, against the plain batch call and, record for record, against the host harness that runs the same core
(tests/emul/nfa_set_resume_emul.cpp), on the corpus and the cuts of tests/test_nfa_set_resume_cpu.py (tests/testlib.py,
tests/setwalk_lib.py); every mask width; the sticky errors; no result bytes; streams and capture; the host entry point."""
import numpy as np
import pytest

import oracle_lib
from mfa_amd import capi, image
from setwalk_lib import (INVALID, LANE_WORDS, LIVE, START, check_records_are_clean, feed_records, new_records, piece_rounds, record, records_of, records_view,
                         run_lane_pieces, whole)
from testlib import MAX_BYTES, NFA_NAMES, ROUNDS, blob_of, emul_exe, expected, filled, front_end_blob, k_regex, match_on_gpu, rnd, seen_so_far, setwalk_corpus, upload, wide_images, wide_strings

pytestmark = pytest.mark.gpu


@pytest.fixture()
def env(monkeypatch):
    for k in ("MFA_NFA_SETWALK", "MFA_DFA_STATE_LIMIT"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


@pytest.fixture(scope="module")
def emul():
    return emul_exe("nfa_set_resume")


def forced(env, blob):
    """the blob's image as a set-walk image, whatever its number of state sets"""
    env.setenv("MFA_NFA_SETWALK", "1")
    img = capi.Image(blob)
    env.delenv("MFA_NFA_SETWALK")
    assert img.info()["dfa_states"] == 0
    return img


def mismatch(got, want, strings, what):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s: %d mismatches, first string %d (len %d) want %d got %d" % (what, bad.size, bad[0], len(strings[bad[0]]), want[bad[0]], got[bad[0]])


def bookkeeping(img):
    assert img.info()["last_kernel"] == capi.KERNEL_NODESET
    assert img.last_dfa_split() == (0, 0, 0) and img.last_dfa_spec() == (0, 0, 0) and img.last_kernel_ms() > 0.0


def pieces_against_whole(img, emul, tmp_path, blob, strings, want, rng, what):
    """the strings cut as tests/test_nfa_set_resume_cpu.py cuts them and fed in ROUNDS rounds in scan order: every round's results against the
    oracle on what has been given so far; the final records, word for word, against ONE call on the whole strings from zeroed records
    and against the records the host harness prints; that call's results against mfa_match_batch.  Returns the whole strings' records"""
    n = len(strings)
    n_nodes = image.blob_info(blob)["n_nodes"]
    rounds, is_rev = piece_rounds(blob, strings, rng)
    ora = oracle_lib.OracleImage(blob)
    d_states = new_records(n, LANE_WORDS)
    for r in range(ROUNDS):
        got = feed_records(img, [s[b:e] for s, (b, e) in zip(strings, rounds[r])], d_states, LANE_WORDS)
        mismatch(got, want if r == ROUNDS - 1 else ora.match(seen_so_far(strings, rounds, r, is_rev)), strings, "%s round %d" % (what, r))
    bookkeeping(img)
    d_whole = new_records(n, LANE_WORDS)
    res_whole = feed_records(img, strings, d_whole, LANE_WORDS)
    recs, recs_whole = records_of(d_states, n, LANE_WORDS), records_of(d_whole, n, LANE_WORDS)
    _, recs_host = run_lane_pieces(emul, tmp_path, blob, strings, whole(strings))
    assert np.array_equal(recs, recs_whole) and np.array_equal(recs_whole, recs_host), what
    check_records_are_clean(recs, n_nodes, LANE_WORDS)
    assert (recs[:, 0] == LIVE).all()
    assert np.array_equal(res_whole, match_on_gpu(img, strings, exact=True)[0]) and np.array_equal(res_whole, want), what
    bookkeeping(img)
    return recs_whole


def fewer_than_a_wave(img, strings, want, recs_whole, what):
    """the last 45 strings as a batch of their own, in two rounds"""
    few = list(range(len(strings) - 45, len(strings)))
    is_rev = img.info()["is_reversed"]
    halves = [[strings[k][:len(strings[k]) // 2] for k in few], [strings[k][len(strings[k]) // 2:] for k in few]]
    d_states = new_records(45, LANE_WORDS)
    for pieces in (halves[::-1] if is_rev else halves):
        got = feed_records(img, pieces, d_states, LANE_WORDS)
    mismatch(got, want[few], [strings[k] for k in few], what + " (45 strings)")
    assert np.array_equal(records_of(d_states, 45, LANE_WORDS), recs_whole[few]), what


@pytest.mark.parametrize("rev", [0, 1], ids=["forward", "reversed"])
@pytest.mark.parametrize("name", NFA_NAMES)
def test_piecewise_parity(env, emul, name, rev, tmp_path):
    blob, strings, golden = setwalk_corpus(name, rev)
    want = expected(blob, strings, golden)
    assert len(strings) % 256 != 0 and len(strings) > 512 and max(len(s) for s in strings) <= 4096
    img = forced(env, blob)
    what = "%s rev %d" % (name, rev)
    recs_whole = pieces_against_whole(img, emul, tmp_path, blob, strings, want, np.random.default_rng(len(name) * 977 + rev), what)
    fewer_than_a_wave(img, strings, want, recs_whole, what)


def test_wider_masks_and_deep_chains(env, emul, tmp_path):
    """two, four and eight mask words and epsilon chains that need the stack, created with a low tabulation limit so that they fall over by
    themselves; and the k = 10 Thompson image (2050 state sets) under a limit of 1000.  (The k = 20 image is not created here: 2.4 s and
    several hundred MB per creation, and tests/test_nfa_setwalk_gpu.py pays that once.)"""
    rng = np.random.default_rng(80)
    blobs = wide_images(tmp_path)
    env.setenv("MFA_DFA_STATE_LIMIT", "2")
    images = {key: capi.Image(blob) for key, blob in blobs.items()}
    blobs["k10"] = front_end_blob(k_regex(10), tmp_path, 0, "-thompson")
    env.setenv("MFA_DFA_STATE_LIMIT", "1000")
    images["k10"] = capi.Image(blobs["k10"])
    env.delenv("MFA_DFA_STATE_LIMIT")
    for key, img in images.items():
        strings = wide_strings(rng, 600) if key != "k10" else [rnd(b"ab", int(ln), rng) for ln in rng.integers(0, 300, size=596)] + [b"a" + b"b" * 10, b"b" + b"a" * 10, b"", b"abc" + b"a" * 30]
        want = oracle_lib.OracleImage(blobs[key]).match(strings)
        assert 0 < int(want.sum()) < len(strings) and img.info()["dfa_states"] == 0, key
        recs_whole = pieces_against_whole(img, emul, tmp_path, blobs[key], strings, want, rng, key)
        fewer_than_a_wave(img, strings, want, recs_whole, key)


def test_sticky_errors_and_dead_on_entry(env):
    """an unknown tag, INVALID on entry, a bit for a node the image lacks (inside its mask width, and in a word beyond it), a reserved word
    that is not zero and a piece of MFA_MAX_STRING_BYTES + 1 bytes (not walked, so it costs nothing): result 2, tag INVALID and zero
    nodes, again after a following valid piece; a record that enters dead leaves dead with result 0 although its piece is valid text; the
    neighbours in the batch are matched.  A piece of EXACTLY the limit is not tested here: one lane would walk 16 MiB"""
    import torch
    blob = blob_of("nfa_abb_thompson", 0)
    img = forced(env, blob)
    n_nodes = img.info()["n_nodes"]
    assert n_nodes < 32 and not img.info()["is_reversed"]
    big = torch.full((MAX_BYTES + 1 + 64 + 16,), ord("a"), dtype=torch.uint8, device="cuda")
    head = b"aabb" * 5                                                             # strings 0-4: aabb each
    big[:len(head)] = torch.tensor(list(head), dtype=torch.uint8)
    e = len(head) + MAX_BYTES + 1                                                  # string 5: limit + 1 bytes of a
    tail = b"abb" + b"abb" + b"aa"                                                 # strings 6, 7, 8
    big[e:e + len(tail)] = torch.tensor(list(tail), dtype=torch.uint8)
    off = torch.tensor([0, 4, 8, 12, 16, 20, e, e + 3, e + 6, e + 8], dtype=torch.int64, device="cuda")
    rows = np.stack([record(LANE_WORDS, 2), record(LANE_WORDS, INVALID), record(LANE_WORDS, LIVE, [1 << n_nodes]), record(LANE_WORDS, LIVE, [1, 0, 0, 0, 0, 0, 0, 1]),
                     record(LANE_WORDS, START, [], (0, 0, 9)), record(LANE_WORDS, START), record(LANE_WORDS, LIVE), record(LANE_WORDS, START),
                     record(LANE_WORDS, START, [0xdeadbeef] * 8)])
    n = len(rows)
    d_states = new_records(n, LANE_WORDS, rows)
    res = filled(n)
    img.match_tensors_resume_set(big, off, records_view(d_states, n, LANE_WORDS), res)
    torch.cuda.synchronize()
    recs = records_of(d_states, n, LANE_WORDS)
    assert list(res.cpu().numpy()) == [2] * 6 + [0, 1, 0]
    assert (recs[:6, 0] == INVALID).all() and not recs[:6, 1:].any() and list(recs[6]) == [LIVE] + [0] * 11
    assert recs[7, 0] == LIVE and recs[8, 0] == LIVE and recs[7, 4] != 0 and recs[8, 4] != 0
    check_records_are_clean(recs, n_nodes, LANE_WORDS)
    # a valid piece for every string: the errors stay, the dead stays, the others go on ("abb" + "abb" is accepted, "aa" + "ab" is not)
    got = feed_records(img, [b"abb"] * 8 + [b"ab"], d_states, LANE_WORDS)
    recs = records_of(d_states, n, LANE_WORDS)
    assert list(got) == [2] * 6 + [0, 1, 0]
    assert (recs[:6, 0] == INVALID).all() and not recs[:6, 1:].any() and list(recs[6]) == [LIVE] + [0] * 11 and recs[8, 4] != 0
    check_records_are_clean(recs, n_nodes, LANE_WORDS)
    del big
    torch.cuda.empty_cache()


def test_no_result_bytes_on_intermediate_rounds(env):
    """d_results == NULL on the first two of three rounds: the last round's answers are the oracle's on the whole strings"""
    blob = blob_of("nfa_abb_glushkov", 0)
    rng = np.random.default_rng(6)
    strings = [rnd(b"ab", int(ln), rng) + t for ln, t in zip(rng.integers(0, 2000, size=300), [b"abb", b"ab", b"", b"abz"] * 75)]
    img = forced(env, blob)
    thirds = [[s[k * len(s) // 3:(k + 1) * len(s) // 3] for s in strings] for k in range(3)]
    if img.info()["is_reversed"]:
        thirds = thirds[::-1]
    d_states = new_records(len(strings), LANE_WORDS)
    assert feed_records(img, thirds[0], d_states, LANE_WORDS, results=False) is None
    assert feed_records(img, thirds[1], d_states, LANE_WORDS, results=False) is None
    got = feed_records(img, thirds[2], d_states, LANE_WORDS)
    want = oracle_lib.OracleImage(blob).match(strings)
    assert 0 < int(want.sum()) < len(strings)
    mismatch(got, want, strings, "no result bytes")


def test_two_streams_one_image(env):
    """one image, two streams, two batches of the same shape and different content in flight at once, three rounds each"""
    import torch
    blob = blob_of("nfa_abb_thompson", 0)
    rng = np.random.default_rng(78)
    lens = [3000, 50, 2999, 0, 1, 999, 16, 17] + [int(x) for x in rng.integers(0, 3001, size=292)]
    ora = oracle_lib.OracleImage(blob)
    img = forced(env, blob)
    assert not img.info()["is_reversed"]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    work = []
    for v in range(2):
        strings = [rnd(b"ab", ln, rng) for ln in lens]
        strings = [s[:-3] + b"abb" if (k + v) % 2 and len(s) >= 3 else s for k, s in enumerate(strings)]
        rounds = [upload([s[r * len(s) // 3:(r + 1) * len(s) // 3] for s in strings], exact=True) for r in range(3)]
        work.append((rounds, new_records(len(lens), LANE_WORDS), filled(len(lens)), ora.match(strings)))
    assert not np.array_equal(work[0][3], work[1][3])
    torch.cuda.synchronize()
    for r in range(3):
        for v in range(2):
            rounds, d_states, res, _ = work[v]
            img.match_tensors_resume_set(rounds[r][0], rounds[r][1], records_view(d_states, len(lens), LANE_WORDS), res if r == 2 else None, stream=streams[v])
    torch.cuda.synchronize()
    for rounds, d_states, res, want in work:
        assert np.array_equal(res.cpu().numpy(), want)


def test_resume_set_call_is_capturable(env):
    """as tests/test_dfa_resume_gpu.py::test_resume_call_is_capturable: after a first uncaptured call (it allocates the workspace and raises
    the kernel's LDS limit), the call is captured on one stream (no parallel branches) and replayed twice with new records and new bytes
    in the same buffers"""
    import torch
    blob = blob_of("nfa_abb_glushkov", 0)
    rng = np.random.default_rng(13)
    first = [rnd(b"ab", int(ln), rng) for ln in [3000, 2, 2999, 3, 0] + [int(x) for x in rng.integers(0, 3001, size=295)]]
    second = [rnd(b"ab", len(s), rng) for s in first]
    second[0] = second[0][:-3] + b"abb"
    second[3] = b"bab"
    img = forced(env, blob)
    assert not img.info()["is_reversed"]
    joined = [a + b for a, b in zip(first, second)]
    ora = oracle_lib.OracleImage(blob)
    want_first, want_joined = ora.match(first), ora.match(joined)
    assert 0 < int(want_first.sum()) < len(first) and 0 < int(want_joined.sum()) < len(first) and not np.array_equal(want_first, want_joined)
    d_bytes, d_off, _ = upload(first, exact=True)
    d_states = records_view(new_records(len(first), LANE_WORDS), len(first), LANE_WORDS)
    res = filled(len(first))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        img.match_tensors_resume_set(d_bytes, d_off, d_states, res)
    torch.cuda.synchronize()
    assert np.array_equal(res.cpu().numpy(), want_first)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        img.match_tensors_resume_set(d_bytes, d_off, d_states, res)
    torch.cuda.synchronize()
    for pieces, want in ((first, want_first), (second, want_joined)):      # replay 1: the first pieces again from zeroed records; replay 2: the second pieces on top
        if pieces is first:
            d_states.zero_()
        data, _ = oracle_lib.pack(pieces)
        d_bytes[:len(data)] = torch.from_numpy(data.copy()).cuda()
        res.fill_(7)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(res.cpu().numpy(), want)


def test_host_entry_point(env):
    """mfa_match_batch_resume_set_host: two rounds with host pointers, no result bytes in the first"""
    blob = blob_of("nfa_abb_thompson", 0)
    strings = [b"ab" * 50 + b"abb", b"abb", b"", b"abz" * 9, b"b" * 700 + b"abb"]
    img = forced(env, blob)
    assert not img.info()["is_reversed"]
    states = np.zeros(len(strings) * LANE_WORDS, dtype=np.uint32)
    d1, o1 = oracle_lib.pack([s[:len(s) // 2] for s in strings])
    d2, o2 = oracle_lib.pack([s[len(s) // 2:] for s in strings])
    assert img.match_host_resume_set(np.concatenate([d1, np.zeros(16, np.uint8)]), o1, states, want_results=False) is None
    got = img.match_host_resume_set(np.concatenate([d2, np.zeros(16, np.uint8)]), o2, states)
    assert list(got) == list(oracle_lib.OracleImage(blob).match(strings)) == [1, 1, 0, 0, 1]
    recs = states.reshape(len(strings), LANE_WORDS)
    check_records_are_clean(recs, img.info()["n_nodes"], LANE_WORDS)
    assert list(recs[:, 0]) == [LIVE] * 5 and list(recs[3]) == [LIVE] + [0] * 11      # "abz...": dead
    bookkeeping(img)
