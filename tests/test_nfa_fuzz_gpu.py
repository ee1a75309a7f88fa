"""The memory-less engines on automata nobody has seen before, on the GPU: what the host builds of their cores (tests/test_nfa_fuzz_cpu.py)
cannot see -- 64 lanes, the LDS fill from a byte_class of up to 200 classes, tile staging, the queue hand-over of the split paths, the
NLIT selects of the SGPR-packed kernel, a table reload between automata with different alphabets.

One fixed corpus (tests/nfa_fuzz.py: gpu_corpus, seed 0): raw random automata with labels from all bytes but '.', letter edges to lower
ranks and 2 to 130 nodes, and regex-derived ones, with about 240 strings each sampled from the automaton itself, 16 of them pumped to 256 -
3 000 bytes and starting at every offset mod 16.  Every batch has a length that is no multiple of 64, is uploaded with exactly the room
the 16-byte read rule asks for, and is answered into a buffer prefilled with 7 with 64 guard bytes behind it.  Every comparison is exact."""
import numpy as np
import pytest

import nfa_fuzz
import setresume_lib
import testlib
from mfa_amd import capi
from test_dfa_spec_gpu import prime
from test_walk_fuzz_gpu import GUARD, answers, guarded, segment_sizes
from testlib import ROUNDS, cuts_for, expected_split, feed, new_states, pieces_against_whole, rounds_of, states_of

pytestmark = pytest.mark.gpu

KNOBS = ("MFA_DFA_KERNEL", "MFA_DFA_SPLIT_MIN", "MFA_DFA_CHUNK", "MFA_DFA_SPLIT", "MFA_DFA_SPEC", "MFA_NFA_SETWALK", "MFA_DFA_STATE_LIMIT", "MFA_MIXED_DFA",
         "MFA_MIXED_DFA_OWN", "MFA_WALK")


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
def setwalk_images():
    return [next((k, im) for k, im in enumerate(corpus()) if nfa_fuzz.mask_words(im["info"]) == w and im["info"]["is_reversed"] == rev)
            for w in (1, 2, 4, 8) for rev in (0, 1)]


@pytest.mark.parametrize("k,im", setwalk_images(), ids=["%d-words-%s" % (w, d) for w in (1, 2, 4, 8) for d in ("fwd", "rev")])
def test_set_walk(k, im, env):
    """MFA_NFA_SETWALK=1 on one image per mask width and direction: the whole call, and mfa_match_batch_resume_set in ROUNDS rounds --
    the last round's answers and the records against one call on the whole strings"""
    img = forced(im, env)
    strings, n = im["strings"], len(im["strings"])
    d_bytes, d_off, _ = upload(strings)
    compare(call(img, d_bytes, d_off, n, "set walk"), im, "set walk")
    assert img.info()["last_kernel"] == capi.KERNEL_NODESET
    rounds, is_rev = setresume_lib.piece_rounds(im["blob"], strings, np.random.default_rng(2000 + k))
    d_states = setresume_lib.new_records(n)
    for r in range(ROUNDS):
        got = setresume_lib.feed_set(img, [s[b:e] for s, (b, e) in zip(strings, rounds[r])], d_states)
    compare(got, im, "set walk in pieces")
    d_whole = setresume_lib.new_records(n)
    compare(setresume_lib.feed_set(img, strings, d_whole), im, "set walk, whole strings through the resume call")
    recs = setresume_lib.records_of(d_states, n)
    assert np.array_equal(recs, setresume_lib.records_of(d_whole, n))
    setresume_lib.check_records_are_clean(recs, im["info"]["n_nodes"])
    assert img.info()["last_kernel"] == capi.KERNEL_NODESET
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
