"""Wave images on strings given in pieces, on the GPU: mfa_match_batch_resume_set_wide (nfa_set_wave_resume_kernel, csrc/nfa_set_wave.hip)
against the CPU restatement, against the plain batch call and, record for record, against the host harness that runs the same core
(tests/emul/nfa_set_wave_resume_emul.cpp), on the images, strings and cuts of tests/test_nfa_set_wave_resume_cpu.py (tests/setwalk_lib.py);
both placements of the tables; batch shapes that leave waves idle and that make the persistent loop run; the sticky errors; no result bytes; the lane kernel's records; streams and capture; the host entry point; the command line."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib
from mfa_amd import capi, image
from setwalk_lib import (COUNTER300, LANE_MAX_NODES, LANE_WORDS, LIVE, N_ROUNDS, RAW_NODES, WIDE_WORDS, call_records, check_records_are_clean, check_sticky, feed_records,
                         fixed_cuts, new_records, pieces_of, raw_corpus_once, records_of, records_view, regex_strings, results_of, run_wide_pieces, sticky_case, tables_in_lds,
                         three_rounds, wide_regex_images)
from testlib import DIPLOMA, blob_of, emul_exe, front_end_blob, match_on_gpu, rnd, seen_so_far, upload, wide_images, wide_strings

pytestmark = pytest.mark.gpu

REGEX_IMAGES = ("k_512", "k_512_rev", "k_1024", "k_2048", "deep")


@pytest.fixture()
def env(monkeypatch):
    for k in ("MFA_NFA_SETWALK", "MFA_DFA_STATE_LIMIT", "MFA_SET_WAVE", "MFA_SET_SPLIT", "DIPLOMA_PIECE_BYTES"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


@pytest.fixture(scope="module")
def emul():
    return emul_exe("nfa_set_wave_resume")


def regex_image(env, blob):
    """created with a low tabulation limit, so it falls over to the set walk by itself -- and, beyond 256 nodes, to the wave kernel"""
    env.setenv("MFA_DFA_STATE_LIMIT", "2")
    img = capi.Image(blob)
    env.delenv("MFA_DFA_STATE_LIMIT")
    assert img.info()["dfa_states"] == 0 and img.info()["n_nodes"] > LANE_MAX_NODES and img.resume_state_bytes() == 4 * WIDE_WORDS
    return img


def set_walk_image(env, blob, wave=False):
    env.setenv("MFA_NFA_SETWALK", "1")
    if wave:
        env.setenv("MFA_SET_WAVE", "1")
    img = capi.Image(blob)
    env.delenv("MFA_NFA_SETWALK")
    env.delenv("MFA_SET_WAVE", raising=False)
    assert img.info()["dfa_states"] == 0
    return img


def raw_by_nodes():
    """n_nodes -> (name, blob, strings, want): one image per node count of the raw corpus, the directions taking turns"""
    corpus, dropped = raw_corpus_once(RAW_NODES, 2)
    assert 10 * dropped <= len(corpus) + dropped
    out = {}
    for k, n_nodes in enumerate(RAW_NODES):
        have = [c for c in corpus if image.blob_info(c[1])["n_nodes"] == n_nodes]
        assert have, n_nodes
        out[n_nodes] = have[k % 2 if len(have) > 1 else 0]
    assert {image.blob_info(c[1])["reversed"] for c in out.values()} == {0, 1}
    return out


def mismatch(got, want, strings, what):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s: %d mismatches, first string %d (len %d) want %d got %d" % (what, bad.size, bad[0], len(strings[bad[0]]), want[bad[0]], got[bad[0]])


def bookkeeping(img):
    assert img.info()["last_kernel"] == capi.KERNEL_NODESET
    assert img.last_set_split() == (0, 0, 0, 0, 0, 0) and img.last_dfa_split() == (0, 0, 0) and img.last_dfa_spec() == (0, 0, 0) and img.last_kernel_ms() > 0.0


def pieces_against_harness(img, emul, tmp_path, blob, strings, rounds, is_rev, want, what):
    """the strings fed in N_ROUNDS rounds in scan order, each round's batch in exactly the room the read rule asks for: every round's
    results against the oracle on what has been given so far; the final records, bit for bit, against the records the host harness
    prints for the whole strings; guard quarters around the records and guard bytes around the results untouched (records_of,
    results_of).  Returns the harness's "tables" line"""
    n = len(strings)
    ora = oracle_lib.OracleImage(blob)
    buf = new_records(n, WIDE_WORDS)
    for r in range(N_ROUNDS):
        got = feed_records(img, pieces_of(strings, rounds[r]), buf, WIDE_WORDS)
        mismatch(got, want if r == N_ROUNDS - 1 else ora.match(seen_so_far(strings, rounds, r, is_rev)), strings, "%s round %d" % (what, r))
    bookkeeping(img)
    recs = records_of(buf, n, WIDE_WORDS)
    tables, digits, recs_host = run_wide_pieces(emul, tmp_path, blob, [strings])
    assert np.array_equal(digits[0], want), what
    assert np.array_equal(recs, recs_host), what
    check_records_are_clean(recs, image.blob_info(blob)["n_nodes"], WIDE_WORDS)
    assert (recs[:, 0] == LIVE).all()
    return tables


def whole_equals_plain(img, strings, want, what):
    """one round through the wide call from zeroed records: byte for byte what mfa_match_batch answers on the same image"""
    got = feed_records(img, strings, new_records(len(strings), WIDE_WORDS), WIDE_WORDS)
    plain = match_on_gpu(img, strings, exact=True)[0]
    assert np.array_equal(got, plain) and np.array_equal(got, want), what


# ---- answers and records --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", REGEX_IMAGES)
def test_piecewise_parity_regex_images(env, emul, name, tmp_path):
    blob, alphabet, min_len = wide_regex_images(tmp_path)[name]
    rng = np.random.default_rng(len(name))
    strings = regex_strings(rng, alphabet, min_len)
    want = oracle_lib.OracleImage(blob).match(strings)
    assert 0 < int(want.sum()) < len(strings)
    img = regex_image(env, blob)
    rounds, is_rev = three_rounds(blob, strings, rng)
    pieces_against_harness(img, emul, tmp_path, blob, strings, rounds, is_rev, want, name)
    whole_equals_plain(img, strings, want, name)
    pick = lambda ln: bytes(rng.choice(list(alphabet), size=int(ln)).tolist())
    strings, rounds = fixed_cuts(pick, is_rev)
    want = oracle_lib.OracleImage(blob).match(strings)
    assert 0 < int(want.sum()) < len(strings)
    pieces_against_harness(img, emul, tmp_path, blob, strings, rounds, is_rev, want, name + ", fixed cuts")


@pytest.mark.parametrize("n_nodes", RAW_NODES)
def test_piecewise_parity_raw_images(env, emul, n_nodes, tmp_path):
    name, blob, strings, want = raw_by_nodes()[n_nodes]
    img = set_walk_image(env, blob)
    assert img.info()["n_nodes"] == n_nodes and img.resume_state_bytes() == 4 * WIDE_WORDS
    rounds, is_rev = three_rounds(blob, strings, np.random.default_rng(n_nodes))
    pieces_against_harness(img, emul, tmp_path, blob, strings, rounds, is_rev, want, name)
    whole_equals_plain(img, strings, want, name)


def test_both_table_placements(emul, tmp_path):
    """the images of the two parity tests above keep their tables behind the stacks in LDS, and read them through L2, in both scan
    directions: all four instantiations of the kernel are walked.  The placement is the harness's printed table words and depth,
    (4 * depth + words) * 4 against 65536"""
    images = wide_regex_images(tmp_path)
    cases = [(name, images[name][0]) for name in REGEX_IMAGES] + [(c[0], c[1]) for c in raw_by_nodes().values()]
    seen = {}
    for name, blob in cases:
        words, _, depth = run_wide_pieces(emul, tmp_path, blob, [[b"ab"]])[0]
        seen.setdefault((image.blob_info(blob)["reversed"], (4 * depth + words) * 4 <= 65536), []).append(name)
    assert set(seen) == {(0, True), (0, False), (1, True), (1, False)}, seen
    assert "k_512" in seen[(0, True)] and "k_2048" in seen[(0, False)] and "deep" in seen[(1, True)]


# ---- shapes ---------------------------------------------------------------------------------------------------------------------------
def test_grid_edges(env, emul, tmp_path):
    """1 and 5 strings: waves of a block beyond n; and more strings than resident waves, three times n_cus * lds_blocks_per_cu * 4 plus
    one, of 0 to 8 bytes over two rounds: every wave takes several records in its loop"""
    import torch
    name, blob, strings, want = raw_corpus_once(RAW_NODES, 2)[0][0]
    info = image.blob_info(blob)
    assert info["n_nodes"] == 257 and info["reversed"] == 0
    img = set_walk_image(env, blob)
    ora = oracle_lib.OracleImage(blob)
    acc, rej = np.nonzero(want == 1)[0], np.nonzero(want == 0)[0]
    order = [acc[0], rej[0], acc[1], rej[1], acc[2]]
    for n in (1, 5):
        pick = [strings[int(k)] for k in order[:n]]
        buf = new_records(n, WIDE_WORDS)
        feed_records(img, [s[:len(s) // 2] for s in pick], buf, WIDE_WORDS, results=False)
        got = feed_records(img, [s[len(s) // 2:] for s in pick], buf, WIDE_WORDS)
        mismatch(got, want[order[:n]], pick, "%s, %d strings" % (name, n))
        assert (records_of(buf, n, WIDE_WORDS)[:, 0] == LIVE).all()
    emul_tables = run_wide_pieces(emul, tmp_path, blob, [[b"ab"]])[0]
    lds = (4 * emul_tables[2] + (emul_tables[0] if tables_in_lds(emul_tables) else 0)) * 4
    per_cu = min(8, max(1, (160 * 1024) // max(lds, 1)))
    n = 3 * torch.cuda.get_device_properties(0).multi_processor_count * per_cu * 4 + 1
    short = [strings[k % len(strings)][:(k // len(strings)) % 9] for k in range(n)]      # prefixes: the image scans forward
    assert max(len(s) for s in short) == 8 and min(len(s) for s in short) == 0
    buf = new_records(n, WIDE_WORDS)
    first = feed_records(img, [s[:len(s) // 2] for s in short], buf, WIDE_WORDS)
    mismatch(first, ora.match([s[:len(s) // 2] for s in short]), short, name + ", many short strings, round 0")
    got = feed_records(img, [s[len(s) // 2:] for s in short], buf, WIDE_WORDS)
    mismatch(got, ora.match(short), short, name + ", many short strings")
    recs = records_of(buf, n, WIDE_WORDS)
    check_records_are_clean(recs, 257, WIDE_WORDS)
    whole = new_records(n, WIDE_WORDS)
    feed_records(img, short, whole, WIDE_WORDS)
    assert np.array_equal(recs, records_of(whole, n, WIDE_WORDS))
    bookkeeping(img)


# ---- the record's checks ------------------------------------------------------------------------------------------------------------------
def test_sticky_errors_and_dead_on_entry(env, tmp_path):
    """the records of tests/test_nfa_set_wave_resume_cpu.py::test_record_checks_on_the_harness on the device, mixed among good strings in
    one batch: result 2, tag INVALID and zero nodes, again after an ordinary piece; the dead record leaves dead with result 0; the
    offsets of the dead and the over-long record point outside the batch, whose room is exactly what the read rule asks for"""
    import torch
    blob = front_end_blob(COUNTER300, tmp_path)
    env.setenv("MFA_DFA_STATE_LIMIT", "100")
    img = capi.Image(blob)
    env.delenv("MFA_DFA_STATE_LIMIT")
    assert img.info()["n_nodes"] == 303 and img.info()["dfa_states"] == 0 and not img.info()["is_reversed"]
    rows, rounds, _, _, _, _ = sticky_case()
    n = len(rows)
    buf = new_records(n, WIDE_WORDS, rows)
    digits, recs = [], []
    for _, off, data in rounds:
        d_bytes = torch.zeros((len(data) + 15) // 16 * 16, dtype=torch.uint8, device="cuda")
        d_bytes[:len(data)] = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy())
        d_off = torch.from_numpy(np.asarray(off, dtype=np.int64)).cuda()
        res = call_records(img, d_bytes, d_off, buf, n, WIDE_WORDS)
        torch.cuda.synchronize()
        digits.append(results_of(res, n))
        recs.append(records_of(buf, n, WIDE_WORDS))
    check_sticky(blob, digits, recs, "device")
    bookkeeping(img)


def test_no_result_bytes_on_intermediate_rounds(env, tmp_path):
    """d_results == NULL on the first two of three rounds: the last round's answers are the oracle's on the whole strings"""
    blob, alphabet, min_len = wide_regex_images(tmp_path)["k_512_rev"]
    rng = np.random.default_rng(6)
    strings = [rnd(alphabet, int(ln), rng) for ln in rng.integers(0, 700, size=200)]
    img = regex_image(env, blob)
    assert img.info()["is_reversed"]
    thirds = [[s[k * len(s) // 3:(k + 1) * len(s) // 3] for s in strings] for k in range(3)][::-1]
    buf = new_records(len(strings), WIDE_WORDS)
    assert feed_records(img, thirds[0], buf, WIDE_WORDS, results=False) is None
    assert feed_records(img, thirds[1], buf, WIDE_WORDS, results=False) is None
    got = feed_records(img, thirds[2], buf, WIDE_WORDS)
    want = oracle_lib.OracleImage(blob).match(strings)
    assert 0 < int(want.sum()) < len(strings)
    mismatch(got, want, strings, "no result bytes")


# ---- two kernels, one answer --------------------------------------------------------------------------------------------------------------
def test_wide_records_equal_the_lane_records(env, tmp_path):
    """narrow images under MFA_NFA_SETWALK=1, once as lane images and once with MFA_SET_WAVE=1, fed the same pieces: the results agree,
    nodes[0..7] of the wide records are `nodes` of the 48-byte records of mfa_match_batch_resume_set, nodes[8..63] are zero"""
    rng = np.random.default_rng(21)
    blobs = dict(wide_images(tmp_path))
    blobs["abb"] = blob_of("nfa_abb_thompson", 0)
    blobs["abb_rev"] = blob_of("nfa_abb_thompson", 1)
    for key, blob in blobs.items():
        strings = wide_strings(rng) if key not in ("abb", "abb_rev") else [rnd(b"ab", int(ln), rng) + t for ln, t in zip(rng.integers(0, 500, size=200), [b"abb", b"ab", b"", b"abz"] * 50)]
        if key == "abb_rev":
            strings = [s[::-1] for s in strings]
        want = oracle_lib.OracleImage(blob).match(strings)
        assert 0 < int(want.sum()) < len(strings), key
        lane, wave = set_walk_image(env, blob), set_walk_image(env, blob, wave=True)
        assert (lane.resume_state_bytes(), wave.resume_state_bytes()) == (48, 272)
        rounds, is_rev = three_rounds(blob, strings, rng)
        n = len(strings)
        d_lane, buf = new_records(n, LANE_WORDS), new_records(n, WIDE_WORDS)
        for r in range(N_ROUNDS):
            pieces = pieces_of(strings, rounds[r])
            got_lane, got_wave = feed_records(lane, pieces, d_lane, LANE_WORDS), feed_records(wave, pieces, buf, WIDE_WORDS)
            assert np.array_equal(got_lane, got_wave), "%s round %d" % (key, r)
        mismatch(got_wave, want, strings, key)
        recs_lane, recs = records_of(d_lane, n, LANE_WORDS), records_of(buf, n, WIDE_WORDS)
        assert np.array_equal(recs[:, :12], recs_lane) and not recs[:, 12:].any(), key


# ---- streams, capture, host pointers ------------------------------------------------------------------------------------------------------
def test_two_streams_one_image(env):
    """one image, two streams, two batches of the same shape and different content in flight at once, three rounds each"""
    import torch
    name, blob, strings, want = raw_by_nodes()[513]
    is_rev = image.blob_info(blob)["reversed"]
    img = set_walk_image(env, blob)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    n = 120
    work = []
    for v in range(2):
        mine = strings[v * n:(v + 1) * n]
        thirds = [[s[k * len(s) // 3:(k + 1) * len(s) // 3] for s in mine] for k in range(3)]
        rounds = [upload(p, exact=True) for p in (thirds[::-1] if is_rev else thirds)]
        work.append((rounds, new_records(n, WIDE_WORDS), want[v * n:(v + 1) * n]))
    assert not np.array_equal(work[0][2], work[1][2])
    torch.cuda.synchronize()
    res = [None, None]
    for r in range(3):
        for v in range(2):
            rounds, buf, _ = work[v]
            out = call_records(img, rounds[r][0], rounds[r][1], buf, n, WIDE_WORDS, results=r == 2, stream=streams[v])
            if r == 2:
                res[v] = out
    torch.cuda.synchronize()
    for v in range(2):
        assert np.array_equal(results_of(res[v], n), work[v][2])
        assert (records_of(work[v][1], n, WIDE_WORDS)[:, 0] == LIVE).all()


def test_wide_call_is_capturable(env, tmp_path):
    """as tests/test_nfa_set_resume_gpu.py::test_resume_set_call_is_capturable: after a first uncaptured call (it allocates the workspace
    and raises the kernel's LDS limit), the call is captured on ONE stream (no parallel branches) and replayed twice with new records
    and new bytes in the same buffers"""
    import torch
    blob, alphabet, min_len = wide_regex_images(tmp_path)["k_512"]
    rng = np.random.default_rng(13)
    first = [rnd(alphabet, int(ln), rng) for ln in [700, 2, 699, 3, 0] + [int(x) for x in rng.integers(0, 701, size=195)]]
    second = [rnd(alphabet, len(s), rng) for s in first]
    img = regex_image(env, blob)
    assert not img.info()["is_reversed"]
    joined = [a + b for a, b in zip(first, second)]
    ora = oracle_lib.OracleImage(blob)
    want_first, want_joined = ora.match(first), ora.match(joined)
    assert 0 < int(want_first.sum()) < len(first) and 0 < int(want_joined.sum()) < len(first) and not np.array_equal(want_first, want_joined)
    n = len(first)
    d_bytes, d_off, _ = upload(first, exact=True)
    buf = new_records(n, WIDE_WORDS)
    view = records_view(buf, n, WIDE_WORDS)
    res = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        img.match_tensors_resume_set_wide(d_bytes, d_off, view, res)
    torch.cuda.synchronize()
    assert np.array_equal(res.cpu().numpy(), want_first)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        img.match_tensors_resume_set_wide(d_bytes, d_off, view, res)
    torch.cuda.synchronize()
    for pieces, want in ((first, want_first), (second, want_joined)):      # replay 1: the first pieces again from zeroed records; replay 2: the second pieces on top
        if pieces is first:
            view.zero_()
        data, _ = oracle_lib.pack(pieces)
        d_bytes[:len(data)] = torch.from_numpy(data.copy()).cuda()
        res.fill_(7)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(res.cpu().numpy(), want)
    assert (records_of(buf, n, WIDE_WORDS)[:, 0] == LIVE).all()


def test_host_entry_point(env, tmp_path):
    """mfa_match_batch_resume_set_wide_host: two rounds with host pointers, no result bytes in the first"""
    blob = front_end_blob(COUNTER300, tmp_path)
    env.setenv("MFA_DFA_STATE_LIMIT", "100")
    img = capi.Image(blob)
    env.delenv("MFA_DFA_STATE_LIMIT")
    strings = [b"a" * 300, b"a" * 299, b"", b"a" * 150 + b"b" + b"a" * 149, b"a" * 900]
    states = np.zeros(len(strings) * WIDE_WORDS, dtype=np.uint32)
    d1, o1 = oracle_lib.pack([s[:len(s) // 2] for s in strings])
    d2, o2 = oracle_lib.pack([s[len(s) // 2:] for s in strings])
    assert img.match_host_resume_set_wide(np.concatenate([d1, np.zeros(16, np.uint8)]), o1, states, want_results=False) is None
    got = img.match_host_resume_set_wide(np.concatenate([d2, np.zeros(16, np.uint8)]), o2, states)
    assert list(got) == list(oracle_lib.OracleImage(blob).match(strings)) == [1, 0, 1, 0, 1]
    recs = states.reshape(len(strings), WIDE_WORDS)
    check_records_are_clean(recs, 303, WIDE_WORDS)
    assert list(recs[:, 0]) == [LIVE] * 5 and list(recs[3]) == [LIVE] + [0] * (WIDE_WORDS - 1)      # the string with a `b`: dead
    bookkeeping(img)


# ---- the command line -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [[], ["-reverse"]], ids=["forward", "reverse"])
def test_command_line_in_pieces(env, tmp_path, flags):
    """`diploma -match` on (a^300)* under a limit of 100 state sets with DIPLOMA_PIECE_BYTES=1024: strings beyond 1024 bytes go through
    Automata's match_in_pieces, which asks mfa_image_resume_state_bytes and takes the wide call; the oracle's answers, and the same
    answers without the knob through the plain call (a line of the command line carries no empty string)"""
    lens = [300, 299, 600, 1, 1024, 1025, 1200, 1500, 2048, 2049, 2100, 3000, 3001, 4500, 5000, 4999]
    words = ["a" * ln for ln in lens] + ["a" * 1500 + "b" + "a" * 1499, "b" + "a" * 2999, "a" * 2999 + "b"]
    p = subprocess.run([DIPLOMA, "-dump"], input=COUNTER300 + "\n", capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode == 0, p.stderr
    blob = image.blob_from_dump(p.stdout)
    assert image.blob_info(blob)["n_nodes"] > LANE_MAX_NODES
    want = [int(x) for x in oracle_lib.OracleImage(blob).match([w.encode() for w in words])]
    assert want == [1 if ln % 300 == 0 else 0 for ln in lens] + [0, 0, 0]
    e = {k: v for k, v in os.environ.items() if k not in ("MFA_NFA_SETWALK", "MFA_SET_WAVE", "DIPLOMA_PIECE_BYTES")}
    e.update(MFA_DFA_STATE_LIMIT="100", MFA_VERBOSE="1")
    text = COUNTER300 + "\n" + "\n".join(words) + "\nexit\n"
    r = subprocess.run([DIPLOMA, "-match"] + flags, input=text, capture_output=True, text=True, cwd=tmp_path, env=dict(e, DIPLOMA_PIECE_BYTES="1024"))
    assert r.returncode == 0, r.stderr
    assert [int(x) for x in r.stdout.split() if x in ("0", "1")] == want
    assert "nfa_set_wave_resume_kernel" in r.stderr
    r = subprocess.run([DIPLOMA, "-match"] + flags, input=text, capture_output=True, text=True, cwd=tmp_path, env=e)
    assert r.returncode == 0, r.stderr
    assert [int(x) for x in r.stdout.split() if x in ("0", "1")] == want
    assert "nfa_set_wave_kernel" in r.stderr and "nfa_set_wave_resume_kernel" not in r.stderr
