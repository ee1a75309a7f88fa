"""The memory-less engines on automata nobody has seen before, on the GPU: what the host builds of their cores (tests/test_nfa_fuzz_cpu.py)
cannot see -- 64 lanes, the LDS fill from a byte_class of up to 200 classes, tile staging, the queue hand-over of the split paths, the
NLIT selects of the SGPR-packed kernel, a table reload between automata with different alphabets.

One fixed corpus (tests/nfa_fuzz.py: gpu_corpus, seed 0): raw random automata with labels from all bytes but '.', letter edges to lower
ranks and 2 to 130 nodes, and regex-derived ones, with about 240 strings each sampled from the automaton itself, 16 of them pumped to 256 -
3 000 bytes and starting at every offset mod 16.  Every batch has a length that is no multiple of 64, is uploaded with exactly the room
the 16-byte read rule asks for, and is answered into a buffer prefilled with 7 with 64 guard bytes behind it.  Every comparison is exact.

The set walk (section d) takes every image of nfa_fuzz.set_corpus(0), forced to the node set: the lane kernels whole, in pieces, with
long strings cut (plain and RESUME form of csrc/nfa_set_split.hip) and the wave kernels under MFA_SET_WAVE=1 -- every mask width in both
directions, and tables in LDS and through L2 in both directions; the test ids say which."""
import numpy as np
import pytest

import nfa_fuzz
import setwalk_lib
import testlib
from mfa_amd import capi
from test_dfa_spec_gpu import prime
from test_walk_fuzz_gpu import GUARD, answers, guarded, segment_sizes
from testlib import ROUNDS, cuts_for, emul_exe, expected_split, feed, new_states, pieces_against_whole, rounds_of, states_of

pytestmark = pytest.mark.gpu

KNOBS = ("MFA_DFA_KERNEL", "MFA_DFA_SPLIT_MIN", "MFA_DFA_CHUNK", "MFA_DFA_SPLIT", "MFA_DFA_SPEC", "MFA_NFA_SETWALK", "MFA_DFA_STATE_LIMIT", "MFA_MIXED_DFA",
         "MFA_MIXED_DFA_OWN", "MFA_WALK", "MFA_SET_WAVE", "MFA_SET_SPLIT", "MFA_SET_SPLIT_ROUNDS", "MFA_SET_SPLIT_LOOKBACK")


@pytest.fixture()
def env(monkeypatch):
    """no knob set on entry; monkeypatch deletes every knob a test set when it ends"""
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def corpus():
    return nfa_fuzz.gpu_corpus()


def states(im):
    return im["info"]["dfa_states"]


def ids(images):
    return ["%d-%dsets-%dcls-%s" % (k, states(im), im["info"]["byte_classes"], "rev" if im["info"]["is_reversed"] else "fwd") for k, im in images]


def every(has):
    images = [(k, im) for k, im in enumerate(corpus()) if has(im)]
    return pytest.mark.parametrize("k,im", images, ids=ids(images))


def image_of(im, env):
    """the image as the library makes it; one whose state sets pass nfa_fuzz.PROBE_LIMIT is made a set-walk image at once (tabulating it to
    the default limit of 2^20 sets takes seconds and hundreds of MB, and where that ends is not this corpus's business)"""
    if not states(im):
        return forced(im, env)
    img = capi.Image(im["blob"])
    assert img.info()["dfa_states"] == states(im) and img.info()["byte_classes"] == im["info"]["byte_classes"]
    return img


def forced(im, env):
    env.setenv("MFA_NFA_SETWALK", "1")
    img = capi.Image(im["blob"])
    env.delenv("MFA_NFA_SETWALK")
    assert img.info()["dfa_states"] == 0
    return img


def upload(strings):
    return testlib.upload(strings, exact=True)


def call(img, d_bytes, d_off, n, what):
    buf = guarded(n)
    img.match_tensors(d_bytes, d_off, buf)
    return answers(buf, n, what)


def compare(got, im, what):
    bad = np.nonzero(got != im["want"])[0]
    assert bad.size == 0, "%s, %s: %d of %d strings wrong, first %r (len %d) want %d got %d" % (
        im["what"], what, bad.size, len(got), im["strings"][bad[0]][:60], len(im["strings"][bad[0]]), im["want"][bad[0]], got[bad[0]])


def test_the_corpus_is_what_the_tests_count_on():
    c = corpus()
    nfa_fuzz.report(c, 0)
    nfa_fuzz.check_lines(c)
    nfa_fuzz.report_set(set_corpus(), 0)
    nfa_fuzz.check_set_lines(set_corpus())
    assert GUARD == 64


# ---- a. the plain call ----------------------------------------------------------------------------------------------------------------
@every(lambda im: True)
def test_plain_call(k, im, env):
    """Default knobs, MFA_DFA_KERNEL=simple, MFA_DFA_KERNEL=packed.  Under `packed` launch_dfa takes the SGPR form when make_packed
    succeeds -- at most 8 state sets and 8 byte classes, every literal class one byte, which holds for every image (nfa_byte_classes) --
    and n_lit = byte_classes - 1 is at most 4: dfa_tiled_kernel<REV, true, NLIT, false> with NLIT = byte_classes - 1, the corpus's lines
    "packed, 0 .. 4 literal classes" in both directions; "5 or more" falls through to the LDS form.  (The ABI cannot report which ran.)
    128 to 254 state sets: MFA_ERR_UNSUPPORTED, and nothing written."""
    import torch
    img = image_of(im, env)
    d_bytes, d_off, _ = upload(im["strings"])
    n = len(im["strings"])
    got = []
    for mode in (None, "simple", "packed"):
        if mode:
            env.setenv("MFA_DFA_KERNEL", mode)
        what = "MFA_DFA_KERNEL=%s" % mode
        if 128 <= states(im) <= 254:
            buf = guarded(n)
            with pytest.raises(capi.MfaError) as err:
                img.match_tensors(d_bytes, d_off, buf)
            torch.cuda.synchronize()
            assert err.value.code == capi.ERR_UNSUPPORTED and (buf.cpu().numpy() == 7).all(), what
            continue
        got.append(call(img, d_bytes, d_off, n, what))
        compare(got[-1], im, what)
        assert np.array_equal(got[-1], got[0]), what
        assert img.info()["last_kernel"] == (capi.KERNEL_TABLE if states(im) else capi.KERNEL_NODESET)
    img.close()


# ---- b. long strings: the split path and the L2 table's ---------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [16, 48])
@every(lambda im: 2 <= states(im) <= 127 or states(im) >= 255)
def test_split_and_spec_paths(k, im, chunk, env):
    """MFA_DFA_SPLIT_MIN=256 and chunks of 16 or 48 bytes: the batch's pumped strings, which start at every offset mod 16, are cut.  Up to
    127 state sets: dfa_split.hip, on either side of split_lanes_log2's border at 64.  255 and more: dfa_spec.hip on a primed workspace,
    then with MFA_DFA_SPEC=0.  mfa_last_dfa_split reports the header's formulas; the answers are the oracle's and those of MFA_DFA_SPLIT=0."""
    env.setenv("MFA_DFA_SPLIT_MIN", "256")
    env.setenv("MFA_DFA_CHUNK", str(chunk))
    img = image_of(im, env)
    d_bytes, d_off, off = upload(im["strings"])
    n = len(im["strings"])
    cut = expected_split(off, 256, chunk)
    assert cut[0] >= 16 and cut[2] == chunk
    if states(im) >= 255:
        prime(img)
    got = call(img, d_bytes, d_off, n, "chunk %d" % chunk)
    compare(got, im, "MFA_DFA_SPLIT_MIN=256 MFA_DFA_CHUNK=%d" % chunk)
    assert img.last_dfa_split() == cut
    if states(im) >= 255:
        env.setenv("MFA_DFA_SPEC", "0")
        plain = call(img, d_bytes, d_off, n, "MFA_DFA_SPEC=0")
        assert img.last_dfa_split() == (0, 0, 0) and img.last_dfa_spec() == (0, 0, 0)
        compare(plain, im, "MFA_DFA_SPEC=0")
    env.setenv("MFA_DFA_SPLIT", "0")
    plain = call(img, d_bytes, d_off, n, "MFA_DFA_SPLIT=0")
    assert img.last_dfa_split() == (0, 0, 0)
    compare(plain, im, "MFA_DFA_SPLIT=0")
    assert np.array_equal(got, plain)
    img.close()


# ---- c. strings in pieces -----------------------------------------------------------------------------------------------------------------
@every(lambda im: states(im) >= 2)
def test_resume(k, im, env):
    """testlib.pieces_against_whole on every tabulated image.  128 to 254 state sets, which mfa_match_batch refuses: the same rounds, the
    last round and one call on the whole strings against the oracle and against each other (tests/test_dfa_resume_gpu.py:
    test_table_between_lds_and_l2)"""
    img = image_of(im, env)
    strings, rng = im["strings"], np.random.default_rng(1000 + k)
    if not 128 <= states(im) <= 254:
        pieces_against_whole(img, im["blob"], strings, rng, im["what"])
        return
    n = len(strings)
    rounds = rounds_of(strings, cuts_for(strings, rng), im["info"]["is_reversed"])
    d_states = new_states(n)
    for r in range(ROUNDS):
        got = feed(img, [s[b:e] for s, (b, e) in zip(strings, rounds[r])], d_states)
    compare(got, im, "pieces")
    d_whole = new_states(n)
    compare(feed(img, strings, d_whole), im, "whole strings through the resume call")
    assert np.array_equal(states_of(d_states, n), states_of(d_whole, n)) and int(states_of(d_whole, n).max()) < states(im)


# ---- d. the set walk ------------------------------------------------------------------------------------------------------------------------
def set_corpus():
    return nfa_fuzz.set_corpus(0)


def every_set():
    """every image of the set corpus; the id carries mask width, direction and table placement"""
    images = list(enumerate(set_corpus()))
    return pytest.mark.parametrize("k,im", images, ids=[nfa_fuzz.set_id(k, im) for k, im in images])


@every_set()
def test_set_walk(k, im, env):
    """MFA_NFA_SETWALK=1 on every image of the set corpus, so on every mask width in both directions with the tables in LDS, and on W 4
    and W 8 in both directions with the tables read through L2 (30 237 and 188 546 table words; the forward ones are direction twins):
    the whole call, and mfa_match_batch_resume_set in ROUNDS rounds -- the last round's answers and the records against one call on the
    whole strings"""
    img = forced(im, env)
    strings, n = im["strings"], len(im["strings"])
    d_bytes, d_off, _ = upload(strings)
    compare(call(img, d_bytes, d_off, n, "set walk"), im, "set walk")
    assert img.info()["last_kernel"] == capi.KERNEL_NODESET
    rounds, is_rev = setwalk_lib.piece_rounds(im["blob"], strings, np.random.default_rng(2000 + k))
    d_states = setwalk_lib.new_records(n, setwalk_lib.LANE_WORDS)
    for r in range(ROUNDS):
        got = setwalk_lib.feed_records(img, [s[b:e] for s, (b, e) in zip(strings, rounds[r])], d_states, setwalk_lib.LANE_WORDS)
    compare(got, im, "set walk in pieces")
    d_whole = setwalk_lib.new_records(n, setwalk_lib.LANE_WORDS)
    compare(setwalk_lib.feed_records(img, strings, d_whole, setwalk_lib.LANE_WORDS), im, "set walk, whole strings through the resume call")
    recs = setwalk_lib.records_of(d_states, n, setwalk_lib.LANE_WORDS)
    assert np.array_equal(recs, setwalk_lib.records_of(d_whole, n, setwalk_lib.LANE_WORDS))
    setwalk_lib.check_records_are_clean(recs, im["info"]["n_nodes"], setwalk_lib.LANE_WORDS)
    assert img.info()["last_kernel"] == capi.KERNEL_NODESET
    img.close()


SPLIT_MIN = 256                                          # MFA_DFA_SPLIT_MIN of the tests below: the corpus's pumped strings are cut
ZEROS = (0, 0, 0, 0, 0, 0)
WAVE_ARENA = 32768                                       # the most chunks a wave image's workspace reserves (nfa_set_wave_split_core.h)


def long_only(im):
    """the image's strings of SPLIT_MIN bytes and more, and the oracle's answers for them: a batch the host harnesses of the split paths
    cut exactly as the kernels do (they cut every string)"""
    keep = [j for j, s in enumerate(im["strings"]) if len(s) >= SPLIT_MIN]
    assert len(keep) >= 16 and len(keep) % 64 != 0
    return [im["strings"][j] for j in keep], im["want"][keep]


def compare_long(got, want, strings, im, what):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s, %s: %d of %d long strings wrong, first (len %d) want %d got %d" % (im["what"], what, bad.size, len(strings), len(strings[bad[0]]), want[bad[0]], got[bad[0]])


@pytest.mark.parametrize("chunk", [16, 48])
@every_set()
def test_set_split(k, im, chunk, env, tmp_path):
    """MFA_DFA_SPLIT_MIN=256 and chunks of 16 or 48 bytes on every image forced to the set walk: nfa_set_kernel queues the batch's pumped
    strings, which start at every offset mod 16, and csrc/nfa_set_split.hip cuts them -- the oracle's answers, the header's formulas in
    mfa_last_set_split, zeros in mfa_last_dfa_split and mfa_last_dfa_spec; MFA_SET_SPLIT=0 answers the same bytes and reports six zeros.
    Then the long strings alone under (rounds, lookback) of (0, 0), (3, 64) and (1, 8): the oracle's answers, and the counts of chunks
    walked again, of strings resolved serially and of their bytes are those of the host harness on the same batch and settings.  On
    random automata those counts run into the thousands (tests/test_nfa_fuzz_cpu.py: test_set_split_core has the figures)."""
    env.setenv("MFA_DFA_SPLIT_MIN", str(SPLIT_MIN))
    env.setenv("MFA_DFA_CHUNK", str(chunk))
    img = forced(im, env)
    d_bytes, d_off, off = upload(im["strings"])
    n = len(im["strings"])
    cut = expected_split(off, SPLIT_MIN, chunk)
    assert cut[0] >= 16 and cut[2] == chunk
    got = call(img, d_bytes, d_off, n, "chunk %d" % chunk)
    compare(got, im, "MFA_DFA_SPLIT_MIN=256 MFA_DFA_CHUNK=%d" % chunk)
    assert img.last_set_split()[:3] == cut
    assert img.last_dfa_split() == (0, 0, 0) and img.last_dfa_spec() == (0, 0, 0) and img.info()["last_kernel"] == capi.KERNEL_NODESET
    env.setenv("MFA_SET_SPLIT", "0")
    plain = call(img, d_bytes, d_off, n, "MFA_SET_SPLIT=0")
    assert img.last_set_split() == ZEROS and img.last_dfa_split() == (0, 0, 0) and img.last_dfa_spec() == (0, 0, 0)
    compare(plain, im, "MFA_SET_SPLIT=0")
    assert np.array_equal(got, plain)
    env.delenv("MFA_SET_SPLIT")
    longs, want = long_only(im)
    d_bytes, d_off, off = upload(longs)
    cut = expected_split(off, SPLIT_MIN, chunk)
    assert cut[0] == len(longs)
    for rounds, lookback in ((0, 0), (3, 64), (1, 8)):
        what = "long strings only, chunk %d rounds %d lookback %d" % (chunk, rounds, lookback)
        env.setenv("MFA_SET_SPLIT_ROUNDS", str(rounds))
        env.setenv("MFA_SET_SPLIT_LOOKBACK", str(lookback))
        compare_long(call(img, d_bytes, d_off, len(longs), what), want, longs, im, what)
        report = img.last_set_split()
        assert report[:3] == cut, (what, report)
        (_, host, digits), = setwalk_lib.run_lane_split(emul_exe("nfa_set_split"), tmp_path, im["blob"], longs, (chunk,), (lookback,), (rounds,))
        assert np.array_equal(digits, want), what
        assert report[3:] == (host["rewalked"], host["serial_strings"], host["serial_bytes"]), (im["what"], what, report, host)
    img.close()


@every_set()
def test_set_split_in_pieces(k, im, env, tmp_path):
    """mfa_match_batch_resume_set under MFA_DFA_SPLIT_MIN=256 and chunks of 16 bytes, the strings in ROUNDS rounds of pieces:
    nfa_set_resume_kernel queues the long pieces of live records and the RESUME forms of csrc/nfa_set_split.hip cut them, each from the
    set its record holds.  On odd rounds below the last every second image is given no result buffer (the resolve kernel writes the
    record alone).  The last round's answers are the oracle's; the records are, word for word, those of one call on the whole strings
    with MFA_SET_SPLIT=0 (the serial kernel) and those of the whole-walk host harness"""
    env.setenv("MFA_DFA_SPLIT_MIN", str(SPLIT_MIN))
    env.setenv("MFA_DFA_CHUNK", "16")
    img = forced(im, env)
    strings, n = im["strings"], len(im["strings"])
    rounds, is_rev = setwalk_lib.piece_rounds(im["blob"], strings, np.random.default_rng(3000 + k))
    assert is_rev == im["info"]["is_reversed"]
    d_states = setwalk_lib.new_records(n, setwalk_lib.LANE_WORDS)
    queued = []
    for r in range(ROUNDS):
        pieces = [s[b:e] for s, (b, e) in zip(strings, rounds[r])]
        got = setwalk_lib.feed_records(img, pieces, d_states, setwalk_lib.LANE_WORDS, results=not (r % 2 == 1 and r < ROUNDS - 1 and k % 2 == 1))
        queued.append(img.last_set_split()[0])
        assert queued[-1] <= sum(1 for p in pieces if len(p) >= SPLIT_MIN) and img.last_dfa_split() == (0, 0, 0) and img.last_dfa_spec() == (0, 0, 0)
    compare(got, im, "split path, strings in pieces")
    assert max(queued) > 0, queued
    recs = setwalk_lib.records_of(d_states, n, setwalk_lib.LANE_WORDS)
    env.setenv("MFA_SET_SPLIT", "0")
    d_whole = setwalk_lib.new_records(n, setwalk_lib.LANE_WORDS)
    compare(setwalk_lib.feed_records(img, strings, d_whole, setwalk_lib.LANE_WORDS), im, "MFA_SET_SPLIT=0, whole strings through the resume call")
    assert img.last_set_split() == ZEROS
    assert np.array_equal(recs, setwalk_lib.records_of(d_whole, n, setwalk_lib.LANE_WORDS))
    digits, recs_host = setwalk_lib.run_lane_pieces(emul_exe("nfa_set_resume"), tmp_path, im["blob"], strings, setwalk_lib.whole(strings))
    assert np.array_equal(digits[0], im["want"]) and np.array_equal(recs, recs_host)
    setwalk_lib.check_records_are_clean(recs, im["info"]["n_nodes"], setwalk_lib.LANE_WORDS)
    assert img.info()["last_kernel"] == capi.KERNEL_NODESET
    img.close()


def forced_wave(im, env):
    env.setenv("MFA_SET_WAVE", "1")
    img = forced(im, env)
    env.delenv("MFA_SET_WAVE")
    assert img.resume_state_bytes() == 4 * setwalk_lib.WIDE_WORDS
    return img


@every_set()
def test_wave_kernels_on_the_corpus(k, im, env, tmp_path):
    """MFA_SET_WAVE=1: the wave kernels (csrc/nfa_set_wave*.hip) on images of 2 to 130 nodes, up to 201 byte classes and labels of 0x80
    and above -- they were made for 257 nodes and more and had met six labels.  The plain call: the oracle's answers, byte for byte the
    lane image's.  mfa_match_batch_resume_set_wide in three rounds of pieces: the last round against the oracle, the wide records
    (guard quarters round them) against one call on the whole strings.  MFA_DFA_SPLIT_MIN=256 and chunks of 48 bytes: the oracle's
    answers, the header's formulas with the wave arena of 32 768 chunks, and on the long strings alone at 3 rounds and a lookback of 64
    the counts of the host harness"""
    lane, img = forced(im, env), forced_wave(im, env)
    assert lane.resume_state_bytes() == 4 * setwalk_lib.LANE_WORDS
    strings, n = im["strings"], len(im["strings"])
    d_bytes, d_off, off = upload(strings)
    got = call(img, d_bytes, d_off, n, "wave")
    compare(got, im, "MFA_SET_WAVE=1")
    assert np.array_equal(got, call(lane, d_bytes, d_off, n, "lane")) and img.last_set_split() == ZEROS and img.info()["last_kernel"] == capi.KERNEL_NODESET
    lane.close()
    # strings in pieces
    rounds, is_rev = setwalk_lib.three_rounds(im["blob"], strings, np.random.default_rng(4000 + k))
    assert is_rev == im["info"]["is_reversed"]
    buf = setwalk_lib.new_records(n, setwalk_lib.WIDE_WORDS)
    for r in range(setwalk_lib.N_ROUNDS):
        got = setwalk_lib.feed_records(img, setwalk_lib.pieces_of(strings, rounds[r]), buf, setwalk_lib.WIDE_WORDS)
    compare(got, im, "MFA_SET_WAVE=1, strings in pieces")
    whole = setwalk_lib.new_records(n, setwalk_lib.WIDE_WORDS)
    compare(setwalk_lib.feed_records(img, strings, whole, setwalk_lib.WIDE_WORDS), im, "MFA_SET_WAVE=1, whole strings through the wide call")
    recs = setwalk_lib.records_of(buf, n, setwalk_lib.WIDE_WORDS)
    assert np.array_equal(recs, setwalk_lib.records_of(whole, n, setwalk_lib.WIDE_WORDS))
    setwalk_lib.check_records_are_clean(recs, im["info"]["n_nodes"], setwalk_lib.WIDE_WORDS)
    # long strings cut
    env.setenv("MFA_DFA_SPLIT_MIN", str(SPLIT_MIN))
    env.setenv("MFA_DFA_CHUNK", "48")
    compare(call(img, d_bytes, d_off, n, "wave, chunk 48"), im, "MFA_SET_WAVE=1 MFA_DFA_SPLIT_MIN=256 MFA_DFA_CHUNK=48")
    cut = expected_split(off, SPLIT_MIN, 48, WAVE_ARENA)
    assert cut[0] >= 16 and cut[2] == 48 and img.last_set_split()[:3] == cut
    assert img.last_dfa_split() == (0, 0, 0) and img.last_dfa_spec() == (0, 0, 0)
    longs, want = long_only(im)
    d_bytes, d_off, off = upload(longs)
    env.setenv("MFA_SET_SPLIT_ROUNDS", "3")
    env.setenv("MFA_SET_SPLIT_LOOKBACK", "64")
    compare_long(call(img, d_bytes, d_off, len(longs), "wave, long only"), want, longs, im, "MFA_SET_WAVE=1, long strings only")
    report = img.last_set_split()
    assert report[:3] == expected_split(off, SPLIT_MIN, 48, WAVE_ARENA) and report[0] == len(longs)
    (_, host, digits), = setwalk_lib.run_wave_split(emul_exe("nfa_set_wave_split"), tmp_path, im["blob"], longs, (48,), (64,), (3,))
    assert np.array_equal(digits, want)
    assert report[3:] == tuple(host[key] for key in setwalk_lib.COUNT_KEYS), (im["what"], report, host)
    img.close()


# ---- e. one mixed object --------------------------------------------------------------------------------------------------------------------
def mixed_images():
    """eleven images whose byte-class maps all differ (their label sets do: nfa_byte_classes numbers the labels): six packed-eligible ones,
    three of 9 to 55 state sets, one the multi-table launch does not take (56 to 127), one walked as a node set; both directions in the
    packed-eligible ones, in those of 9 to 55 state sets and overall.  (kind, corpus index) in segment order."""
    c = corpus()
    out, seen = [], []

    def take(kind, has, count):
        for rev in ([0, 1] * count)[:count]:
            k = next(k for k, im in enumerate(c) if has(im) and im["info"]["is_reversed"] == rev and im["labels"] not in seen)
            seen.append(c[k]["labels"])
            out.append((kind, k))

    take("packed", lambda im: nfa_fuzz.packed(im["info"]), 6)
    take("lds", lambda im: 9 <= states(im) <= 55, 3)
    take("own", lambda im: 56 <= states(im) <= 127, 1)
    take("set", lambda im: nfa_fuzz.mask_words(im["info"]) >= 2 and (states(im) == 0 or states(im) > 254), 1)
    order = [0, 6, 1, 2, 9, 7, 10, 3, 8, 4, 5]               # the kinds interleaved; the empty segment is a packed-eligible image's
    return [out[j] for j in order]


def test_mixed_object(env):
    """Segments of 63, 1, 65, 0, 130, ... strings (tests/test_walk_fuzz_gpu.py: segment_sizes), so that a segment starts inside a wave.
    MFA_MIXED_DFA unset: a launch per non-empty segment.  MFA_MIXED_DFA=1: the images of up to 55 state sets share the multi-table launch,
    whose workgroups reload table and byte classes whenever the automaton changes; mfa_mixed_last_dfa's `strings` counts the strings in
    that launch, so with the strings of the segments that have a launch of their own it is every memory-less string of the batch."""
    c = corpus()
    picks = mixed_images()
    assert 10 <= len(picks) <= 12 and len({tuple(c[k]["labels"]) for _, k in picks}) == len(picks)
    assert {c[k]["info"]["is_reversed"] for kind, k in picks if kind == "packed"} == {0, 1} == {c[k]["info"]["is_reversed"] for kind, k in picks if kind == "lds"}
    sizes = segment_sizes(len(picks))
    strings, seg, want = [], [0], []
    for (kind, k), size in zip(picks, sizes):
        strings += c[k]["strings"][:size]
        want.append(c[k]["want"][:size])
        seg.append(len(strings))
    assert len(strings) % 64 != 0 and {0, 1, 63, 65, 130} <= set(sizes)
    want = np.concatenate(want)
    n = len(strings)
    d_bytes, d_off, _ = upload(strings)
    images = [forced(c[k], env) if kind == "set" else image_of(c[k], env) for kind, k in picks]
    alone = np.concatenate([call(img, d_bytes, d_off[seg[j]:seg[j + 1] + 1], seg[j + 1] - seg[j], ("alone", j)) for j, img in enumerate(images) if seg[j + 1] > seg[j]])
    assert np.array_equal(alone, want), "segment by segment"
    shared = sum(size for (kind, _), size in zip(picks, sizes) if kind in ("packed", "lds"))
    own = sum(1 for (kind, _), size in zip(picks, sizes) if kind in ("own", "set") and size)
    own_strings = sum(size for (kind, _), size in zip(picks, sizes) if kind in ("own", "set"))
    assert own == 2 and shared + own_strings == n
    mx = capi.Mixed(images)
    for multi in (None, "1"):
        if multi:
            env.setenv("MFA_MIXED_DFA", multi)
        buf = guarded(n)
        mx.match_tensors(d_bytes, d_off, seg, d_results=buf)
        what = "MFA_MIXED_DFA=%s" % multi
        got = answers(buf, n, what)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, "%s: %d of %d strings wrong, first string %d %r want %d got %d" % (what, bad.size, n, bad[0], strings[bad[0]][:60], want[bad[0]], got[bad[0]])
        assert np.array_equal(got, alone), what
        d = mx.last_dfa()
        if multi:
            assert d["multi_launches"] >= 1 and d["strings"] == shared and d["own_launches"] == own and d["strings"] + own_strings == n, d
            assert d["items"] == sum(1 for (kind, _), size in zip(picks, sizes) if kind in ("packed", "lds") and size)
        else:
            assert d == {"multi_launches": 0, "own_launches": sum(1 for s in sizes if s), "items": 0, "strings": 0}, d
    mx.close()
    for img in images:
        img.close()
