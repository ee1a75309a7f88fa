#!/usr/bin/env python3
"""The set walk of memory-less automata (nfa_set_kernel) against the table kernels.  One process, the sides of a comparison alternate
call by call, five uncounted rounds, then the median of REPS calls each (default 7, at least 5), kernel time from mfa_last_kernel_ms.
One JSON line per comparison, also appended to profiles/r11_nfa_setwalk.jsonl.

  (a) BASELINE configs[1], 1 Mi x 1 KiB, (a|b)*abb Thompson (nfa_abb_thompson): the tiled table kernel against the forced set walk
  (b) the same batch, (a|b)*a(a|b)^20: the Thompson compile (2^21 state sets: the set walk by itself, four mask words) against the
      Glushkov compile of the same regex (502 609 state sets, asserted to be tabulated: the table kernel with its table in L2).
      Every side's answers are held to the CPU restatement of its own image on the first 1024 strings

  nfa_setwalk.py [REPS] [STRINGS]
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


def main():
    reps = max(5, int(sys.argv[1]) if len(sys.argv) > 1 else 7)
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 1 << 20
    flat, d_off, _ = batch([1024] * n, 2)
    abb = image.blob_from_dump(oracle_lib.load_dump("nfa_abb_thompson"))
    table, _ = created(abb)
    forced, _ = created(abb, "1")
    assert table.info()["dfa_states"] == 6 and forced.info()["dfa_states"] == 0
    compare("(a) %d x 1 KiB, (a|b)*abb" % n, {"table kernel": table, "set walk (forced)": forced}, {"table kernel": abb, "set walk (forced)": abb}, flat, d_off, reps, {})
    regex = "(a|b)*a" + "(a|b)" * 20
    b_thompson, b_glushkov = front_end(regex, "-thompson"), front_end(regex, "-glushkov")
    thompson, t_thompson = created(b_thompson)
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
