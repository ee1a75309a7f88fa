#!/usr/bin/env python3
"""Long strings of memory-less automata whose table lives in L2 (csrc/dfa_spec.hip) against the one-lane walk, (a|b)*a(a|b)^8 (514 state
sets) unless said otherwise.  Kernel time from mfa_last_kernel_ms, two uncounted calls, then the median of REPS calls (default 5); the sides
of a comparison alternate call by call in one process.  "walk" is the same library with MFA_DFA_SPEC=0, which launches the same
main kernel (dfa_spec_big_kernel) with the queue off; MFA_LIB_PATH=<other build> runs any mode against another library for a process-level A/B.
The two sides of "short" therefore run one kernel and differ by a test of split_min alone: that mode is meaningful only with MFA_LIB_PATH pointing
at a build from before the kernels were merged, whose "walk" side is the separate kernel without a queue.
The long-string modes set MFA_DFA_SPLIT=2 on the spec side, so that the workspace's first call is cut like the others (by default it is walked whole).
One JSON line per measurement, appended to OUT (default profiles/r09_dfa_spec.jsonl).

  dfa_spec.py long  [REPS] [OUT]   (a) 8 x 1 MiB, spec against walk; then spec alone: 8 x (16 MiB - 1), and 8 x 1 MiB on 32 770 and 131 074 state sets
  dfa_spec.py short [REPS] [OUT]   (b) 1 Mi x 1 KiB, spec (the main kernel alone: a workspace that has met no long string has no tail) against walk
  dfa_spec.py sweep [REPS] [OUT]   (c) MFA_DFA_SPEC_LOOKBACK 0 / 64 / 256 / 1024 and MFA_DFA_SPEC_ROUNDS 0 / 1 / 3 on (a)
"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "re2-modification_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

from mfa_amd import capi
from testlib import front_end_blob, k_regex

DEV = "cuda:0"


def table(k):
    """(a|b)*a(a|b)^k through the host front-end: 514 state sets at k = 8, 32 770 at 14, 131 074 at 16"""
    with tempfile.TemporaryDirectory() as tmp:
        return capi.Image(front_end_blob(k_regex(k), tmp))


def batch(lens, seed):
    """random text over ab, made on the device"""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    total = int(sum(lens))
    d_bytes = torch.zeros(total + 64, dtype=torch.uint8, device=DEV)
    d_bytes[:total] = torch.randint(0, 2, (total,), generator=g, device=DEV, dtype=torch.uint8) + 97
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    return d_bytes, torch.from_numpy(off).to(DEV), total


def call(img, d_bytes, d_off, res, env):
    for k, v in env.items():
        os.environ[k] = v
    img.match_tensors(d_bytes, d_off, res)
    ms = img.last_kernel_ms()
    for k in env:
        del os.environ[k]
    return ms


def alternate(img, d_bytes, d_off, sides, reps):
    """sides: {name: environment}; every round runs every side once.  Returns per side (times, results, split report, spec report)"""
    n = d_off.numel() - 1
    out = {}
    res = {k: torch.full((n,), 7, dtype=torch.uint8, device=DEV) for k in sides}
    ms = {k: [] for k in sides}
    for r in range(reps + 2):
        for k, env in sides.items():
            t = call(img, d_bytes, d_off, res[k], env)
            if r >= 2:
                ms[k].append(t)
            if r == reps + 1:
                out[k] = (img.last_dfa_split(), img.last_dfa_spec() if hasattr(capi.lib(), "mfa_last_dfa_spec") else None)
    torch.cuda.synchronize()
    first = next(iter(res.values()))
    assert all(torch.equal(first, v) for v in res.values()), "the sides disagree"
    return ms, out


def report(out_path, what, total, ms, did, extra=None):
    line = {"what": what, "device": torch.cuda.get_device_name(0), "lib": os.path.basename(os.path.dirname(capi.LIB_PATH)) + "/" + os.path.basename(capi.LIB_PATH), "bytes": total}
    for k, v in ms.items():
        med = float(np.median(v))
        line[k] = {"kernel_ms": v, "median_ms": med, "spread_ms": float(max(v) - min(v)), "GB/s": total / (med * 1e-3) / 1e9,
                   "split": did[k][0], "spec": did[k][1]}
    line.update(extra or {})
    text = json.dumps(line)
    print(text, flush=True)
    with open(out_path, "a") as f:
        f.write(text + "\n")


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "long"
    reps = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 5
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "r09_dfa_spec.jsonl")
    both = {"spec": {}, "walk": {"MFA_DFA_SPEC": "0"}}
    cut = {"MFA_DFA_SPLIT": "2"}
    if mode == "long":
        img = table(8)
        d_bytes, d_off, total = batch([1 << 20] * 8, 1)
        ms, did = alternate(img, d_bytes, d_off, {"spec": cut, "walk": both["walk"]}, reps)
        report(out_path, "(a) 8 x 1 MiB, 514 state sets", total, ms, did, {"walk/spec": float(np.median(ms["walk"]) / np.median(ms["spec"]))})
        d_bytes, d_off, total = batch([(16 << 20) - 1] * 8, 2)       # (never through the one-lane walk: many seconds a call)
        ms, did = alternate(img, d_bytes, d_off, {"spec": cut}, reps)
        report(out_path, "(a) 8 x (16 MiB - 1), 514 state sets", total, ms, did)
        for k, states in ((14, 32770), (16, 131074)):
            img = table(k)
            d_bytes, d_off, total = batch([1 << 20] * 8, k)
            ms, did = alternate(img, d_bytes, d_off, {"spec": cut}, reps)
            report(out_path, "(a) 8 x 1 MiB, %d state sets" % states, total, ms, did)
    elif mode == "short":
        img = table(8)
        d_bytes, d_off, total = batch([1024] * (1 << 20), 3)
        ms, did = alternate(img, d_bytes, d_off, both, max(reps, 9))
        report(out_path, "(b) 1 Mi x 1 KiB, 514 state sets", total, ms, did, {"spec/walk": float(np.median(ms["spec"]) / np.median(ms["walk"]))})
    elif mode == "sweep":
        img = table(8)
        d_bytes, d_off, total = batch([1 << 20] * 8, 1)
        sides = {"lookback %d" % lb: dict(cut, MFA_DFA_SPEC_LOOKBACK=str(lb)) for lb in (0, 64, 256, 1024)}
        ms, did = alternate(img, d_bytes, d_off, sides, reps)
        report(out_path, "(c) MFA_DFA_SPEC_LOOKBACK on 8 x 1 MiB, 3 rounds", total, ms, did)
        sides = {"rounds %d" % r: dict(cut, MFA_DFA_SPEC_ROUNDS=str(r)) for r in (0, 1, 3)}
        ms, did = alternate(img, d_bytes, d_off, sides, reps)
        report(out_path, "(c) MFA_DFA_SPEC_ROUNDS on 8 x 1 MiB, lookback 256", total, ms, did)
    else:
        sys.exit(__doc__)


if __name__ == "__main__":
    main()
