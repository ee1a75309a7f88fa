#!/usr/bin/env python3
"""Memory-less automata on strings given in pieces (mfa_match_batch_resume) against the plain batch call, (a|b)*abb Thompson NFA
(nfa_abb_thompson).  One process, the two sides of every comparison alternate call by call, median of REPS calls each (default 7, at
least 5), kernel time from mfa_last_kernel_ms.  One JSON line per comparison, also appended to profiles/r08_dfa_resume.jsonl.

  (a) BASELINE configs[1], 1 Mi x 1 KiB, through the resume call in one piece against mfa_match_batch on the same buffers
  (b) the same text as four pieces of 256 B, four calls, against one whole call
  (c) eight strings of 48 MiB - 4 in four pieces each through the resume call against eight of 16 MiB - 1 through mfa_match_batch, per byte
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "re2-modification_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

import oracle_lib
from dfa_long import DEV, LONG, batch
from mfa_amd import capi, image


def states(n):
    return torch.ones(n, dtype=torch.int32, device=DEV)


def alternate(sides, reps):
    """sides: {name: callable returning kernel ms}; five uncounted rounds, then `reps` rounds, every round runs every side once"""
    ms = {k: [] for k in sides}
    for r in range(reps + 5):
        for k, f in sides.items():
            t = f()
            if r >= 5:
                ms[k].append(t)
    return ms


def report(what, ms, bytes_of, extra=None):
    out = {"what": what, "device": torch.cuda.get_device_name(0)}
    for k, v in ms.items():
        med = float(np.median(v))
        out[k] = {"kernel_ms": v, "median_ms": med, "spread_ms": float(max(v) - min(v)), "GB/s": bytes_of[k] / (med * 1e-3) / 1e9}
    out.update(extra or {})
    line = json.dumps(out)
    print(line, flush=True)
    with open(os.path.join(ROOT, "profiles", "r08_dfa_resume.jsonl"), "a") as f:
        f.write(line + "\n")


def main():
    reps = max(5, int(sys.argv[1]) if len(sys.argv) > 1 else 7)
    blob = image.blob_from_dump(oracle_lib.load_dump("nfa_abb_thompson"))
    img = capi.Image(blob)
    # (a), (b): configs[1]
    flat, d_off, want = batch([1024] * (1 << 20), 2)
    n = d_off.numel() - 1
    total = int(d_off[-1])
    res = torch.empty(n, dtype=torch.uint8, device=DEV)
    st = states(n)

    def plain():
        img.match_tensors(flat, d_off, res)
        return img.last_kernel_ms(0)

    def one_piece():
        st.fill_(1)
        img.match_tensors_resume(flat, d_off, st, res)
        return img.last_kernel_ms(0)

    ms = alternate({"mfa_match_batch": plain, "resume, one piece": one_piece}, reps)
    report("(a) 1 Mi x 1 KiB, one piece", ms, {k: total for k in ms}, {"results_exact": bool(torch.equal(res.bool(), want))})
    # the four quarters of every string, each quarter batch packed back to back like the whole
    quarters = [flat[:total].view(n, 4, 256)[:, q, :].contiguous().view(-1) for q in range(4)]
    quarters = [torch.cat([q, torch.zeros(64, dtype=torch.uint8, device=DEV)]) for q in quarters]
    q_off = torch.arange(n + 1, dtype=torch.int64, device=DEV) * 256

    def four_pieces():
        st.fill_(1)
        t = 0.0
        for q in range(4):
            img.match_tensors_resume(quarters[q], q_off, st, res if q == 3 else None)
            t += img.last_kernel_ms(0)
        return t

    ms = alternate({"mfa_match_batch": plain, "resume, four pieces of 256 B": four_pieces}, reps)
    report("(b) 1 Mi x 1 KiB as 4 x 256 B", ms, {k: total for k in ms}, {"results_exact": bool(torch.equal(res.bool(), want))})
    del flat, quarters, res, st
    # (c): long strings
    piece = 12 << 20                                  # four pieces of 12 MiB - 1: a string of 48 MiB - 4
    flat16, off16, want16 = batch([LONG] * 8, 1)
    res16 = torch.empty(8, dtype=torch.uint8, device=DEV)
    pieces = [batch([piece - 1] * 8, 10 + r) for r in range(4)]
    st8 = states(8)
    res8 = torch.empty(8, dtype=torch.uint8, device=DEV)

    def long_plain():
        img.match_tensors(flat16, off16, res16)
        return img.last_kernel_ms(0)

    def long_pieces():
        st8.fill_(1)
        t = 0.0
        for r in range(4):
            img.match_tensors_resume(pieces[r][0], pieces[r][1], st8, res8 if r == 3 else None)
            t += img.last_kernel_ms(0)
        return t

    ms = alternate({"mfa_match_batch, 8 x (16 MiB - 1)": long_plain, "resume, 8 x 4 pieces of 12 MiB - 1": long_pieces}, reps)
    report("(c) long strings, per byte", ms, {"mfa_match_batch, 8 x (16 MiB - 1)": 8 * LONG, "resume, 8 x 4 pieces of 12 MiB - 1": 32 * (piece - 1)},
           {"results_exact": bool(torch.equal(res16.bool(), want16)) and bool(torch.equal(res8.bool(), pieces[3][2])),
            "split(strings,chunks,chunk_bytes)": img.last_dfa_split(0)})


if __name__ == "__main__":
    main()
