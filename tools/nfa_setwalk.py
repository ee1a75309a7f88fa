#!/usr/bin/env python3
"""The set walk of memory-less automata (nfa_set_kernel) against the table kernels.  One process, the sides of a comparison alternate
call by call, five uncounted rounds, then the median of REPS calls each (default 7, at least 5), kernel time from mfa_last_kernel_ms.
One JSON line per comparison, also appended to profiles/r11_nfa_setwalk.jsonl.

  (a) BASELINE configs[1], 1 Mi x 1 KiB, (a|b)*abb Thompson (nfa_abb_thompson): the tiled table kernel against the forced set walk
  (b) the same batch, (a|b)*a(a|b)^20: the Thompson compile (2^21 state sets: the set walk by itself, four mask words) against the
      Glushkov compile of the same regex (502 609 state sets, asserted to be tabulated: the table kernel with its table in L2).
      Every side's answers are held to the CPU restatement of its own image on the first 1024 strings
  (c) strings in pieces: on the two set-walk images of (a) and (b), mfa_match_batch_resume_set on the whole strings from zeroed records
      (nfa_set_resume_kernel: the same step loop, 48 bytes of record in and out per string) against mfa_match_batch on the same batch;
      lines appended to profiles/r12_nfa_set_resume.jsonl.  (An image that says it takes the wide record -- resume_state_bytes() == 272,
      a wave image -- goes through mfa_match_batch_resume_set_wide: `wave resume` below.)

  nfa_setwalk.py [REPS] [STRINGS] [all|tables|resume]      tables: (a) and (b) only; resume: (c) only

  nfa_setwalk.py long sweep|gain|short [REPS] [OUT.jsonl]   long strings cut across the GPU (csrc/nfa_set_split.hip), on (a|b)*abb forced to the
      set walk and on the k = 20 Thompson image; random ab; one JSON line per measurement, appended to OUT.jsonl (default
      profiles/r13_nfa_set_split.jsonl).  Medians of REPS calls (default 7) after five uncounted ones; the answers of the first two
      strings are held to the CPU restatement.
      sweep   8 x 1 MiB and 8 x (16 MiB - 1): MFA_DFA_CHUNK 256 .. 4096 x MFA_SET_SPLIT_LOOKBACK 32 .. 256 x MFA_SET_SPLIT_ROUNDS 0, 3
      gain    8 x 1 MiB with the library's defaults against MFA_SET_SPLIT=0 (the whole walk: one uncounted call and three counted ones, it
              takes seconds per call)
      short   1 Mi x 1 KiB (no long string): this build's kernel time per call, to be set against another build's (MFA_LIB_PATH) process by process

  nfa_setwalk.py long sweep|gain|short REPS OUT.jsonl wave [first] [mib]   the same three for WAVE images (csrc/nfa_set_wave_split.hip), on the
      (a|b)*a(a|b)^k Thompson images of 259 and 1029 nodes (`first`: the 259-node image only); OUT.jsonl is profiles/r16_nfa_set_wave_split.jsonl
      in DESIGN.md
      sweep   8 x 1 MiB: MFA_DFA_CHUNK 256 .. 4096 x MFA_SET_SPLIT_LOOKBACK 32 .. 256 (or those of `lb=64,128,256`) x MFA_SET_SPLIT_ROUNDS 0, 3
      gain    8 x 128 KiB with the library's defaults against MFA_SET_SPLIT=0 (one uncounted call and three counted ones); `mib`: also
              8 x 1 MiB cut (walked whole it takes about a minute of the device per call: not run)
      short   64 Ki x 1 KiB on the 259-node image

  nfa_setwalk.py wave narrow|wide|resume [REPS] [STRINGS] [OUT.jsonl] [first]   the wave-cooperative step (csrc/nfa_set_wave.hip: one string per wave), lines appended
      to OUT.jsonl (default profiles/r14_nfa_set_wave.jsonl).  Medians of REPS calls (default 7) after five uncounted ones, the sides
      alternating; the first strings' answers are held to the CPU restatement.
      narrow  the lane kernel against MFA_SET_WAVE=1 on the same build, on (a|b)*abb forced to the set walk (W = 1) and on the k = 20
              Thompson image (W = 4): STRINGS x 1 KiB (default 1 Mi), 8 192 x 1 KiB, and 8 x 1 MiB with MFA_SET_SPLIT=0 (walked whole:
              one uncounted call and three counted ones)
      wide    images the lane kernel cannot hold: (a|b)*a(a|b)^k Thompson with 257 to 512 and with 1025 to 2048 nodes, STRINGS x 1 KiB;
              bytes per second and per resident wave, and the CPU restatement's time on the first 1024 strings beside it, for scale;
              `first`: the narrower image only (a call on the wider one takes a minute at 1 Mi strings)
      resume  strings in pieces on the two images of `wide`: mfa_match_batch_resume_set_wide on the whole strings from zeroed records
              (nfa_set_wave_resume_kernel: the same walk, 272 bytes of record in and out per string) against mfa_match_batch on the
              same batch, as (c) does for the lane images (five uncounted rounds, REPS at least 3); lines appended to OUT.jsonl
              (default profiles/r15_nfa_set_wave_resume.jsonl)
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "re2-modification_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

import oracle_lib
from dfa_long import DEV, batch
from dfa_resume import alternate
from mfa_amd import capi, image
from testlib import front_end_blob

KERNELS = {capi.KERNEL_TABLE: "table kernel", capi.KERNEL_NODESET: "set walk"}      # what last_kernel says ran, in every output line


def created(blob, setwalk=None):
    """(image, seconds mfa_image_create took); setwalk: the value of MFA_NFA_SETWALK while it is made"""
    old = os.environ.pop("MFA_NFA_SETWALK", None)
    if setwalk is not None:
        os.environ["MFA_NFA_SETWALK"] = setwalk
    t = time.perf_counter()
    img = capi.Image(blob)
    dt = time.perf_counter() - t
    os.environ.pop("MFA_NFA_SETWALK", None)
    if old is not None:
        os.environ["MFA_NFA_SETWALK"] = old
    return img, dt


def front_end(regex, flag):
    return front_end_blob(regex, "/tmp", flag=flag)


SAMPLE = 1024      # strings per side whose answers are held to the CPU restatement of that side's own image


def compare(what, sides, blobs, flat, d_off, reps, extra):
    """sides: name -> image, blobs: name -> its blob.  Every side is checked against the oracle on ITS image: two compiles of one regex
    need not accept the same strings (the reference's skip rule: the Glushkov automaton of (a|b)*a(a|b)^20 rejects about a tenth of
    the strings whose 21st byte from the end is an a)"""
    n = d_off.numel() - 1
    total = int(d_off[-1])
    m = min(n, SAMPLE)
    off = d_off[:m + 1].cpu().numpy().astype(np.uint64)
    data = flat[:int(off[-1])].cpu().numpy()
    want = {k: torch.from_numpy(oracle_lib.OracleImage(blobs[k]).match_packed(data, off).astype(np.uint8)).to(DEV) for k in sides}
    res = {k: torch.full((n,), 7, dtype=torch.uint8, device=DEV) for k in sides}

    def call(k):
        def f():
            sides[k].match_tensors(flat, d_off, res[k])
            return sides[k].last_kernel_ms(0)
        return f

    ms = alternate({k: call(k) for k in sides}, reps)
    out = {"what": what, "device": torch.cuda.get_device_name(0), "strings": n, "bytes": total}
    for k, v in ms.items():
        med = float(np.median(v))
        out[k] = {"kernel_ms": v, "median_ms": med, "spread_ms": float(max(v) - min(v)), "G char-steps/s": total / (med * 1e-3) / 1e9,
                  "results_exact_on_sample": bool(torch.equal(res[k][:m], want[k])), "sample": m, "accepted_in_sample": int(want[k].sum()), "kernel": KERNELS[sides[k].info()["last_kernel"]],
                  "dfa_states": sides[k].info()["dfa_states"]}
    out.update(extra)
    line = json.dumps(out)
    print(line, flush=True)
    with open(os.path.join(ROOT, "profiles", "r11_nfa_setwalk.jsonl"), "a") as f:
        f.write(line + "\n")


def compare_resume(what, img, blob, flat, d_off, reps, out_path=None):
    """the resume call on whole strings from zeroed records against the plain call, one set-walk image, the same batch.  Which resume
    call -- the 48-byte record of a lane image or the 272-byte record of a wave image -- is the image's to say (resume_state_bytes)"""
    n = d_off.numel() - 1
    total = int(d_off[-1])
    m = min(n, SAMPLE)
    off = d_off[:m + 1].cpu().numpy().astype(np.uint64)
    want = torch.from_numpy(oracle_lib.OracleImage(blob).match_packed(flat[:int(off[-1])].cpu().numpy(), off).astype(np.uint8)).to(DEV)
    wide = img.resume_state_bytes() == 4 * capi.SET_STATE_WIDE_WORDS
    words = capi.SET_STATE_WIDE_WORDS if wide else capi.SET_STATE_WORDS
    assert img.resume_state_bytes() == 4 * words
    names = ("mfa_match_batch", "mfa_match_batch_resume_set%s, whole strings from zeroed records" % ("_wide" if wide else ""))
    res = {k: torch.full((n,), 7, dtype=torch.uint8, device=DEV) for k in names}
    d_states = torch.zeros(n * words, dtype=torch.int32, device=DEV)

    def plain():
        img.match_tensors(flat, d_off, res[names[0]])
        return img.last_kernel_ms(0)

    def resume():
        d_states.zero_()                                   # (in front of the start event: not in the kernel's time)
        (img.match_tensors_resume_set_wide if wide else img.match_tensors_resume_set)(flat, d_off, d_states, res[names[1]])
        return img.last_kernel_ms(0)

    ms = alternate({names[0]: plain, names[1]: resume}, reps)
    assert img.info()["dfa_states"] == 0 and img.info()["last_kernel"] == capi.KERNEL_NODESET
    tags = d_states.view(n, words)[:, 0]
    out = {"what": what, "device": torch.cuda.get_device_name(0), "strings": n, "bytes": total, "n_nodes": img.info()["n_nodes"], "record_bytes_in_and_out": 2 * 4 * words * n,
           "results_equal_on_all_strings": bool(torch.equal(res[names[0]], res[names[1]])), "all_records_live": bool((tags == capi.SET_STATE_LIVE).all())}
    for k, v in ms.items():
        med = float(np.median(v))
        out[k] = {"kernel_ms": v, "median_ms": med, "spread_ms": float(max(v) - min(v)), "G char-steps/s": total / (med * 1e-3) / 1e9,
                  "results_exact_on_sample": bool(torch.equal(res[k][:m], want)), "sample": m, "accepted_in_sample": int(want.sum())}
    out["resume_over_plain"] = out[names[1]]["median_ms"] / out[names[0]]["median_ms"]
    line = json.dumps(out)
    print(line, flush=True)
    with open(out_path or os.path.join(ROOT, "profiles", "r12_nfa_set_resume.jsonl"), "a") as f:
        f.write(line + "\n")


_WANT = {}


def long_measure(what, img, blob, flat, d_off, reps, warm, env, out_path):
    """median kernel time of `reps` calls after `warm` uncounted ones under the knobs of `env` (read per call), one JSON line"""
    for k, v in env.items():
        os.environ[k] = str(v)
    n = d_off.numel() - 1
    res = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
    ms = []
    for _ in range(warm + reps):
        img.match_tensors(flat, d_off, res)
        ms.append(img.last_kernel_ms(0))
    report = img.last_set_split(0) if hasattr(capi.lib(), "mfa_last_set_split") else None
    for k in env:
        del os.environ[k]
    m = min(n, 2 if int(d_off[1]) > SAMPLE else SAMPLE)
    off = d_off[:m + 1].cpu().numpy().astype(np.uint64)
    key = (id(blob), flat.data_ptr())
    if key not in _WANT:                                   # (once per image and batch: the sweep comes back to them)
        _WANT[key] = oracle_lib.OracleImage(blob).match_packed(flat[:int(off[-1])].cpu().numpy(), off).astype(np.uint8)[:m]
    want = _WANT[key]
    total = int(d_off[-1])
    med = float(np.median(ms[warm:]))
    out = {"what": what, "device": torch.cuda.get_device_name(0), "strings": n, "bytes": total, "knobs": env, "kernel_ms": ms[warm:], "median_ms": med,
           "spread_ms": float(max(ms[warm:]) - min(ms[warm:])), "MB/s": total / (med * 1e-3) / 1e6, "results_exact_on_sample": bool(np.array_equal(res[:m].cpu().numpy(), want)),
           "sample": m, "set_split(strings,chunks,chunk_bytes,rewalked,serial_strings,serial_bytes)": report, "lib": os.environ.get("MFA_LIB_PATH", "this build"),
           "kernel": KERNELS[img.info()["last_kernel"]]}
    line = json.dumps(out)
    print(line, flush=True)
    with open(out_path, "a") as f:
        f.write(line + "\n")
    return med


def wide_images(first_only=False):
    """[(name, image, blob)]: the (a|b)*a(a|b)^k Thompson images of 259 and 1029 nodes (`wave wide` has them too), wave images by themselves"""
    out = []
    for lo, hi in ((256, 512), (1024, 2048))[:1 if first_only else 2]:
        k = (lo - 9) // 5 + 1                                    # the Thompson compile has 5 k + 9 nodes
        blob = front_end("(a|b)*a" + "(a|b)" * k, "-thompson")
        img, _ = created(blob, "1")
        assert lo < img.info()["n_nodes"] <= hi and img.info()["dfa_states"] == 0 and img.resume_state_bytes() == 4 * capi.SET_STATE_WIDE_WORDS
        out.append(("(a|b)*a(a|b)^%d Thompson, %d nodes" % (k, img.info()["n_nodes"]), img, blob))
    return out


def long_wave_main(mode, reps, out_path):
    """the wave forms of sweep, gain and short (csrc/nfa_set_wave_split.hip); `first` among the arguments: the 259-node image only"""
    images = wide_images("first" in sys.argv[5:] or mode == "short")
    if mode == "short":
        flat, d_off, _ = batch([1024] * (1 << 16), 2)
        for name, img, blob in images:
            long_measure("64 Ki x 1 KiB, " + name, img, blob, flat, d_off, reps, 5, {}, out_path)
        return
    if mode == "gain":
        # 8 x 128 KiB: a whole call is seconds.  (8 x 1 MiB walked whole is about a minute of the device per call: cut only, `mib`)
        small = batch([128 << 10] * 8, 7)
        for name, img, blob in images:
            cut = long_measure("8 x 128 KiB, cut (defaults), " + name, img, blob, small[0], small[1], reps, 5, {}, out_path)
            whole = long_measure("8 x 128 KiB, walked whole, " + name, img, blob, small[0], small[1], 3, 1, {"MFA_SET_SPLIT": 0}, out_path)
            print(json.dumps({"what": "gain, " + name, "whole_over_cut": whole / cut}), flush=True)
        if "mib" in sys.argv[5:]:
            mib = batch([1 << 20] * 8, 5)
            for name, img, blob in images:
                long_measure("8 x 1 MiB, cut (defaults), " + name, img, blob, mib[0], mib[1], reps, 5, {}, out_path)
        return
    mib = batch([1 << 20] * 8, 5)
    # a lookback shorter than the image's memory (k + 1 = 51 and 205 bytes) guesses wrong at every chunk and leaves every string to the
    # serial walk, most of a minute per call: `lb=64,128,256` among the arguments names the lookbacks to sweep
    lookbacks = next(([int(x) for x in a[3:].split(",")] for a in sys.argv[5:] if a.startswith("lb=")), [32, 64, 128, 256])
    for name, img, blob in images:
        for chunk in (256, 512, 1024, 2048, 4096):
            for lookback in lookbacks:
                for rounds in (0, 3):
                    long_measure("8 x 1 MiB, " + name, img, blob, mib[0], mib[1], reps, 5,
                                 {"MFA_DFA_CHUNK": chunk, "MFA_SET_SPLIT_LOOKBACK": lookback, "MFA_SET_SPLIT_ROUNDS": rounds}, out_path)


def long_main():
    mode = sys.argv[2] if len(sys.argv) > 2 else "sweep"
    reps = max(3, int(sys.argv[3])) if len(sys.argv) > 3 else 7
    wave = "wave" in sys.argv[5:]
    out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "r16_nfa_set_wave_split.jsonl" if wave else "r13_nfa_set_split.jsonl")
    assert mode in ("sweep", "gain", "short")
    if wave:
        return long_wave_main(mode, reps, out_path)
    abb = image.blob_from_dump(oracle_lib.load_dump("nfa_abb_thompson"))
    images = [("(a|b)*abb forced to the set walk (W = 1)", created(abb, "1")[0], abb)]
    if mode != "short" or "k20" in sys.argv:
        b20 = front_end("(a|b)*a" + "(a|b)" * 20, "-thompson")
        images.append(("(a|b)*a(a|b)^20 Thompson (W = 4)", created(b20)[0], b20))
    assert all(img.info()["dfa_states"] == 0 for _, img, _ in images)
    if mode == "short":
        flat, d_off, _ = batch([1024] * (1 << 20), 2)
        for name, img, blob in images:
            long_measure("1 Mi x 1 KiB, " + name, img, blob, flat, d_off, reps, 5, {}, out_path)
        return
    mib = batch([1 << 20] * 8, 5)
    if mode == "gain":
        for name, img, blob in images:
            cut = long_measure("8 x 1 MiB, cut (defaults), " + name, img, blob, mib[0], mib[1], reps, 5, {}, out_path)
            whole = long_measure("8 x 1 MiB, walked whole, " + name, img, blob, mib[0], mib[1], 3, 1, {"MFA_SET_SPLIT": 0}, out_path)
            print(json.dumps({"what": "gain, " + name, "whole_over_cut": whole / cut}), flush=True)
        return
    big = batch([(16 << 20) - 1] * 8, 6)
    for name, img, blob in images:
        for label, (flat, d_off, _) in (("8 x 1 MiB", mib), ("8 x (16 MiB - 1)", big)):
            for chunk in (256, 512, 1024, 2048, 4096):
                if (int(d_off[-1]) // 131072 + 15) // 16 * 16 > chunk:      # the arena makes the device choose a larger chunk: the same run as that one
                    continue
                for lookback in (32, 64, 128, 256):
                    for rounds in (0, 3):
                        long_measure("%s, %s" % (label, name), img, blob, flat, d_off, reps, 5,
                                     {"MFA_DFA_CHUNK": chunk, "MFA_SET_SPLIT_LOOKBACK": lookback, "MFA_SET_SPLIT_ROUNDS": rounds}, out_path)


def created_wave(blob, setwalk=None):
    """created() with MFA_SET_WAVE=1 while the image is made: wave tables, whatever its width"""
    os.environ["MFA_SET_WAVE"] = "1"
    try:
        return created(blob, setwalk)[0]
    finally:
        del os.environ["MFA_SET_WAVE"]


def wave_sides(what, sides, blob, flat, d_off, reps, warm, env, out_path, extra=None):
    """sides: name -> image of `blob`; every round runs every side once under the knobs of `env`; one JSON line"""
    for k, v in env.items():
        os.environ[k] = str(v)
    n = d_off.numel() - 1
    total = int(d_off[-1])
    res = {k: torch.full((n,), 7, dtype=torch.uint8, device=DEV) for k in sides}
    ms = {k: [] for k in sides}
    for r in range(warm + reps):
        for k, img in sides.items():
            img.match_tensors(flat, d_off, res[k])
            t = img.last_kernel_ms(0)
            print("  %s, call %d, %s: %.3f ms" % (what, r, k, t), file=sys.stderr, flush=True)      # (a call may take a minute: a sign of life)
            if r >= warm:
                ms[k].append(t)
    for k in env:
        del os.environ[k]
    m = min(n, 2 if int(d_off[1]) > SAMPLE else SAMPLE)
    off = d_off[:m + 1].cpu().numpy().astype(np.uint64)
    t = time.perf_counter()
    want = oracle_lib.OracleImage(blob).match_packed(flat[:int(off[-1])].cpu().numpy(), off).astype(np.uint8)[:m]
    cpu_s = time.perf_counter() - t
    first = next(iter(res.values()))
    out = {"what": what, "device": torch.cuda.get_device_name(0), "strings": n, "bytes": total, "knobs": env,
           "sides_equal_on_all_strings": all(bool(torch.equal(first, v)) for v in res.values()),
           "cpu_restatement": {"strings": m, "bytes": int(off[-1]), "seconds": cpu_s, "MB/s": int(off[-1]) / cpu_s / 1e6}}
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for k, v in ms.items():
        med = float(np.median(v))
        out[k] = {"kernel_ms": v, "median_ms": med, "spread_ms": float(max(v) - min(v)), "MB/s": total / (med * 1e-3) / 1e6,
                  "results_exact_on_sample": bool(np.array_equal(res[k][:m].cpu().numpy(), want)), "sample": m, "accepted_in_sample": int(want.sum()),
                  "kernel": KERNELS[sides[k].info()["last_kernel"]], "n_nodes": sides[k].info()["n_nodes"]}
        if k.startswith("wave"):                               # one string per wave: the rate of one of the waves that run at once (at most 32 per CU)
            out[k]["kB/s per wave"] = total / (med * 1e-3) / 1e3 / min(n, cus * 32)
    if len(ms) == 2:
        a, b = list(ms)
        out["%s over %s" % (b, a)] = out[b]["median_ms"] / out[a]["median_ms"]
    out.update(extra or {})
    line = json.dumps(out)
    print(line, flush=True)
    with open(out_path, "a") as f:
        f.write(line + "\n")


def wave_main():
    mode = sys.argv[2] if len(sys.argv) > 2 else "narrow"
    reps = max(3, int(sys.argv[3])) if len(sys.argv) > 3 else 7
    n = int(sys.argv[4]) if len(sys.argv) > 4 else 1 << 20
    out_path = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "r14_nfa_set_wave.jsonl")
    assert mode in ("narrow", "wide", "resume")
    if mode == "resume" and len(sys.argv) <= 5:
        out_path = os.path.join(ROOT, "profiles", "r15_nfa_set_wave_resume.jsonl")
    kib = batch([1024] * n, 2)
    if mode in ("wide", "resume"):
        for lo, hi in ((256, 512), (1024, 2048))[:1 if "first" in sys.argv[6:] else 2]:
            k = (lo - 9) // 5 + 1                                # the Thompson compile has 5 k + 9 nodes
            blob = front_end("(a|b)*a" + "(a|b)" * k, "-thompson")
            img, _ = created(blob, "1")
            assert lo < img.info()["n_nodes"] <= hi and img.info()["dfa_states"] == 0
            if mode == "resume":
                compare_resume("%d x 1 KiB, (a|b)*a(a|b)^%d Thompson, %d nodes" % (n, k, img.info()["n_nodes"]), img, blob, kib[0], kib[1], reps, out_path)
                continue
            wave_sides("%d x 1 KiB, (a|b)*a(a|b)^%d Thompson, %d nodes" % (n, k, img.info()["n_nodes"]), {"wave kernel": img}, blob, kib[0], kib[1], reps, 5, {}, out_path)
        return
    abb = image.blob_from_dump(oracle_lib.load_dump("nfa_abb_thompson"))
    b20 = front_end("(a|b)*a" + "(a|b)" * 20, "-thompson")
    small = batch([1024] * 8192, 3)
    mib = batch([1 << 20] * 8, 5)
    for name, blob in (("(a|b)*abb forced to the set walk (W = 1)", abb), ("(a|b)*a(a|b)^20 Thompson (W = 4)", b20)):
        sides = {"lane kernel": created(blob, "1")[0], "wave kernel (MFA_SET_WAVE=1)": created_wave(blob, "1")}
        assert all(img.info()["dfa_states"] == 0 for img in sides.values())
        wave_sides("%d x 1 KiB, %s" % (n, name), sides, blob, kib[0], kib[1], reps, 5, {}, out_path)
        wave_sides("8 192 x 1 KiB, " + name, sides, blob, small[0], small[1], reps, 5, {}, out_path)
        wave_sides("8 x 1 MiB, walked whole, " + name, sides, blob, mib[0], mib[1], 3, 1, {"MFA_SET_SPLIT": 0}, out_path)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "long":
        return long_main()
    if len(sys.argv) > 1 and sys.argv[1] == "wave":
        return wave_main()
    reps = max(5, int(sys.argv[1]) if len(sys.argv) > 1 else 7)
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 1 << 20
    which = sys.argv[3] if len(sys.argv) > 3 else "all"
    assert which in ("all", "tables", "resume")
    flat, d_off, _ = batch([1024] * n, 2)
    abb = image.blob_from_dump(oracle_lib.load_dump("nfa_abb_thompson"))
    forced, _ = created(abb, "1")
    regex = "(a|b)*a" + "(a|b)" * 20
    b_thompson = front_end(regex, "-thompson")
    thompson, t_thompson = created(b_thompson)
    if which != "tables":
        compare_resume("(c) %d x 1 KiB, (a|b)*abb forced to the set walk (W = 1)" % n, forced, abb, flat, d_off, reps)
        compare_resume("(c) %d x 1 KiB, (a|b)*a(a|b)^20 Thompson (W = 4)" % n, thompson, b_thompson, flat, d_off, reps)
    if which == "resume":
        return
    table, _ = created(abb)
    assert table.info()["dfa_states"] == 6 and forced.info()["dfa_states"] == 0
    compare("(a) %d x 1 KiB, (a|b)*abb" % n, {"table kernel": table, "set walk (forced)": forced}, {"table kernel": abb, "set walk (forced)": abb}, flat, d_off, reps, {})
    b_glushkov = front_end(regex, "-glushkov")
    glushkov, t_glushkov = created(b_glushkov)
    _, t_thompson_forced = created(b_thompson, "1")
    # the sides are what their names say: Thompson passes the limit, Glushkov (502 609 state sets) does not
    assert thompson.info()["dfa_states"] == 0 and glushkov.info()["dfa_states"] > 0xffff, (thompson.info(), glushkov.info())
    names = ("set walk (Thompson, automatic)", "table kernel, table in L2 (Glushkov)")
    compare("(b) %d x 1 KiB, (a|b)*a(a|b)^20" % n, {names[0]: thompson, names[1]: glushkov}, {names[0]: b_thompson, names[1]: b_glushkov}, flat, d_off, reps,
            {"create_s": {"Thompson (tabulation to the limit, then the set-walk tables)": t_thompson, "Thompson, MFA_NFA_SETWALK=1": t_thompson_forced,
                          "Glushkov (tabulated)": t_glushkov}})


if __name__ == "__main__":
    main()
