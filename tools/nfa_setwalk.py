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
      lines appended to profiles/r12_nfa_set_resume.jsonl

  nfa_setwalk.py [REPS] [STRINGS] [all|tables|resume]      tables: (a) and (b) only; resume: (c) only
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


def compare_resume(what, img, blob, flat, d_off, reps):
    """the resume call on whole strings from zeroed records against the plain call, one set-walk image, the same batch"""
    n = d_off.numel() - 1
    total = int(d_off[-1])
    m = min(n, SAMPLE)
    off = d_off[:m + 1].cpu().numpy().astype(np.uint64)
    want = torch.from_numpy(oracle_lib.OracleImage(blob).match_packed(flat[:int(off[-1])].cpu().numpy(), off).astype(np.uint8)).to(DEV)
    names = ("mfa_match_batch", "mfa_match_batch_resume_set, whole strings from zeroed records")
    res = {k: torch.full((n,), 7, dtype=torch.uint8, device=DEV) for k in names}
    d_states = torch.zeros(n * capi.SET_STATE_WORDS, dtype=torch.int32, device=DEV)

    def plain():
        img.match_tensors(flat, d_off, res[names[0]])
        return img.last_kernel_ms(0)

    def resume():
        d_states.zero_()                                   # (in front of the start event: not in the kernel's time)
        img.match_tensors_resume_set(flat, d_off, d_states, res[names[1]])
        return img.last_kernel_ms(0)

    ms = alternate({names[0]: plain, names[1]: resume}, reps)
    assert img.info()["dfa_states"] == 0 and img.info()["last_kernel"] == capi.KERNEL_NODESET
    tags = d_states.view(n, capi.SET_STATE_WORDS)[:, 0]
    out = {"what": what, "device": torch.cuda.get_device_name(0), "strings": n, "bytes": total, "record_bytes_in_and_out": 2 * 4 * capi.SET_STATE_WORDS * n,
           "results_equal_on_all_strings": bool(torch.equal(res[names[0]], res[names[1]])), "all_records_live": bool((tags == capi.SET_STATE_LIVE).all())}
    for k, v in ms.items():
        med = float(np.median(v))
        out[k] = {"kernel_ms": v, "median_ms": med, "spread_ms": float(max(v) - min(v)), "G char-steps/s": total / (med * 1e-3) / 1e9,
                  "results_exact_on_sample": bool(torch.equal(res[k][:m], want)), "sample": m, "accepted_in_sample": int(want.sum())}
    out["resume_over_plain"] = out[names[1]]["median_ms"] / out[names[0]]["median_ms"]
    line = json.dumps(out)
    print(line, flush=True)
    with open(os.path.join(ROOT, "profiles", "r12_nfa_set_resume.jsonl"), "a") as f:
        f.write(line + "\n")


def main():
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
