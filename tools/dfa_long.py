#!/usr/bin/env python3
"""Long strings of a memory-less automaton: (a|b)*abb Thompson NFA (nfa_abb_thompson) on batches whose time the longest string sets.
Library kernel time (mfa_last_kernel_ms: the table kernel and, behind it, the plan, chunk and fold kernels of the split path).
One JSON line per measurement.  MFA_LIB_PATH selects the library (tools/ab_env.sh), MFA_DFA_SPLIT=0 the path without cutting.

  dfa_long.py long   [REPS]      8 strings of 16 MiB - 1
  dfa_long.py skew   [REPS]      1 Mi strings of 1 KiB with four strings of 16 MiB - 1 scattered through them, and the two parts alone
  dfa_long.py short  [REPS]      BASELINE configs[1]: 1 Mi strings of 1 KiB; also with the split kernels always launched (MFA_DFA_SPLIT=2) and off
  dfa_long.py sweep-min          64 equal strings of 64 KiB .. 4 MiB, cut and not cut: the crossover for MFA_DFA_SPLIT_MIN
  dfa_long.py sweep-chunk        `long` with MFA_DFA_CHUNK = 1 KiB .. 64 KiB
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "re2-modification_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

import oracle_lib
from mfa_amd import capi, image

DEV = torch.device("cuda", 0)
LONG = (16 << 20) - 1


def batch(lens, seed):
    """random strings over ab, every second one ending in abb; returns (bytes, offsets, expected results)"""
    g = torch.Generator(device=DEV); g.manual_seed(seed)
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(np.asarray(lens, dtype=np.int64), out=off[1:])
    total = int(off[-1])
    flat = torch.zeros(total + 64, dtype=torch.uint8, device=DEV)
    flat[:total] = torch.randint(0, 2, (total,), generator=g, device=DEV, dtype=torch.uint8) + ord("a")
    d_off = torch.from_numpy(off).to(DEV)
    ends = d_off[1:][0::2]
    for k, ch in enumerate(b"abb"):
        flat[ends - 3 + k] = ch
    e = d_off[1:]
    want = (flat[e - 3] == ord("a")) & (flat[e - 2] == ord("b")) & (flat[e - 1] == ord("b"))
    return flat, d_off, want


def measure(img, flat, d_off, want, reps, what, extra=None):
    n = d_off.numel() - 1
    res = torch.empty(n, dtype=torch.uint8, device=DEV)
    ms = []
    for _ in range(reps + 5):                       # the first five calls are not counted: the workspace is allocated, and a stream of short strings has dropped the split launches
        res.fill_(7)
        img.match_tensors(flat, d_off, res)
        ms.append(img.last_kernel_ms(0))
    torch.cuda.synchronize()
    split = img.last_dfa_split(0) if hasattr(capi.lib(), "mfa_last_dfa_split") else None
    total = int(d_off[-1])
    t = float(np.median(ms[5:]))
    out = {"what": what, "strings": n, "bytes": total, "kernel_ms": ms[5:], "median_ms": t, "GB/s": total / (t * 1e-3) / 1e9,
           "results_exact": bool(torch.equal(res.bool(), want)), "split(strings,chunks,chunk_bytes)": split,
           "lib": os.environ.get("MFA_LIB_PATH", "this build"), "MFA_DFA_SPLIT": os.environ.get("MFA_DFA_SPLIT", "1"),
           "device": torch.cuda.get_device_name(0)}
    out.update(extra or {})
    print(json.dumps(out), flush=True)
    return t


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "long"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    blob = image.blob_from_dump(oracle_lib.load_dump("nfa_abb_thompson"))
    if mode == "long":
        measure(capi.Image(blob), *batch([LONG] * 8, 1), reps, "8 x (16 MiB - 1)")
    elif mode == "short":
        b = batch([1024] * (1 << 20), 2)
        measure(capi.Image(blob), *b, reps, "1 Mi x 1 KiB")
        if hasattr(capi.lib(), "mfa_last_dfa_split"):      # what the memset and the plan, chunk and fold launches cost when they find nothing
            os.environ["MFA_DFA_SPLIT"] = "2"
            measure(capi.Image(blob), *b, reps, "1 Mi x 1 KiB, split kernels always launched")
            os.environ["MFA_DFA_SPLIT"] = "0"
            measure(capi.Image(blob), *b, reps, "1 Mi x 1 KiB, split path off")
            del os.environ["MFA_DFA_SPLIT"]
    elif mode == "skew":
        lens = [1024] * (1 << 20)
        for at in (1000, 300000, 600000, 1000000):
            lens.insert(at, LONG)
        measure(capi.Image(blob), *batch(lens, 3), reps, "1 Mi x 1 KiB + 4 x (16 MiB - 1)")
        measure(capi.Image(blob), *batch([1024] * (1 << 20), 3), reps, "part: 1 Mi x 1 KiB")
        measure(capi.Image(blob), *batch([LONG] * 4, 3), reps, "part: 4 x (16 MiB - 1)")
    elif mode == "sweep-min":
        for ln in (64 << 10, 128 << 10, 256 << 10, 512 << 10, 1 << 20, 2 << 20, 4 << 20):
            b = batch([ln] * 64, 4)
            for on in ("1", "0"):
                os.environ["MFA_DFA_SPLIT"] = on
                os.environ["MFA_DFA_SPLIT_MIN"] = str(ln)
                measure(capi.Image(blob), *b, reps, "64 x %d KiB" % (ln >> 10), {"cut": on == "1"})
    elif mode == "sweep-chunk":
        b = batch([LONG] * 8, 1)
        for ck in (1 << 10, 2 << 10, 4 << 10, 8 << 10, 16 << 10, 32 << 10, 64 << 10):
            os.environ["MFA_DFA_CHUNK"] = str(ck)
            measure(capi.Image(blob), *b, reps, "8 x (16 MiB - 1)", {"MFA_DFA_CHUNK": ck})
    else:
        sys.exit(__doc__)


if __name__ == "__main__":
    main()
