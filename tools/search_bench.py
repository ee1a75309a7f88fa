#!/usr/bin/env python3
"""Search inside lines (mfa_search_batch) against the whole-string match on the same image, device and batch.  One JSON line per image,
also appended to profiles/r17_search.jsonl.

  LINES (default 1 Mi) lines of 1 KiB of random {a, b}, three images: (a|b)*abb, table_66 = (a|b)*a(a|b)^5 (pass 1 tiled) and table_66
  made to scan from the end (pass 1 of 66 sets: the untiled form).  Per image, alternating call by call:
    match_ms          mfa_match_batch, as the parent commit runs it -- the yardstick: it reads the same bytes once
    results_only_ms   mfa_search_batch without d_spans: pass 1 alone
    with_spans_ms     mfa_search_batch with d_spans and d_span_results: both passes
  mfa_last_kernel_ms of each call, median of REPS (default 20) after three uncounted rounds; the spread is max - min.
  right: the results-only call and the call with spans leave the same result bytes; on the first 2000 lines results and spans equal the
  leftmost-longest match worked out in Python.

  search_bench.py [LINES_Ki] [REPS]
"""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "re2-modification_amd"))

import numpy as np

OUT = os.path.join(ROOT, "profiles", "r17_search.jsonl")
DIPLOMA = os.path.join(ROOT, "re2-modification_amd", "host", "diploma")
AB = "(a|b)"
# name -> (regex, scan from the end, the leftmost-longest match in Python: greedy [ab]* gives back only as far as the last fit of the run)
IMAGES = {"(a|b)*abb": ("(a|b)*abb", 0, rb"[ab]*abb"),
          "table_66": ("(a|b)*a" + AB * 5, 0, rb"[ab]*a[ab]{5}"),
          "table_66 reversed": ("(a|b)*a" + AB * 5, 1, rb"[ab]{5}a[ab]*")}


def blob_of(regex, rev):
    from mfa_amd import image
    p = subprocess.run([DIPLOMA, "-dump", "-thompson"], input=regex + "\n", capture_output=True, text=True, cwd="/tmp", check=True)
    d = image.parse_dump(p.stdout)
    if rev:
        d["reversed"] = 1
    return image.to_blob(d)


def main():
    import torch
    from mfa_amd import capi
    n = (int(sys.argv[1]) if len(sys.argv) > 1 else 1024) << 10
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    assert torch.cuda.is_available(), "search_bench.py measures on a GPU; there is no other way to a time"
    rng = np.random.default_rng(1)
    host = rng.integers(97, 99, size=n * 1024, dtype=np.uint8)
    d_bytes = torch.zeros(host.size + 64, dtype=torch.uint8, device="cuda")
    d_bytes[:host.size] = torch.from_numpy(host)
    d_off = (torch.arange(n + 1, dtype=torch.int64) * 1024).cuda()
    res = [torch.zeros(n, dtype=torch.uint8, device="cuda") for _ in range(3)]
    d_spans = torch.zeros(2 * n + 1, dtype=torch.int64, device="cuda")
    d_sres = torch.zeros(2 * n, dtype=torch.uint8, device="cuda")
    for name, (regex, rev, py) in IMAGES.items():
        img = capi.Image(blob_of(regex, rev))
        calls = {"match_ms": lambda: img.match_tensors(d_bytes, d_off, res[0]),
                 "results_only_ms": lambda: img.search_tensors(d_bytes, d_off, res[1]),
                 "with_spans_ms": lambda: img.search_tensors(d_bytes, d_off, res[2], d_spans, d_sres)}
        times = {k: [] for k in calls}
        for r in range(reps + 3):
            for k, call in calls.items():
                call()
                ms = img.last_kernel_ms()                       # (waits for the call's stop event)
                if r >= 3:
                    times[k].append(ms)
        torch.cuda.synchronize()
        first = min(n, 2000)
        got_res, got_spans = res[2][:first].cpu().numpy(), d_spans[:2 * first].cpu().numpy()
        right = bool(torch.equal(res[1], res[2]))
        for k in range(first):
            m = re.search(py, host[k * 1024:(k + 1) * 1024].tobytes())
            want = (1, k * 1024 + m.start(), k * 1024 + m.end()) if m else (0, k * 1024, k * 1024)
            right = right and (int(got_res[k]), int(got_spans[2 * k]), int(got_spans[2 * k + 1])) == want
        line = {"what": "search inside lines against the whole-string match", "image": name, "device": torch.cuda.get_device_name(0),
                "lines": n, "batch_bytes": int(host.size), "search_tables": list(img.search_info()), "dfa_states": img.info()["dfa_states"], "reps": reps}
        for k, v in times.items():
            line[k] = float(np.median(v))
            line[k.replace("_ms", "_spread_ms")] = float(max(v) - min(v))
            line[k.replace("_ms", "_GB/s")] = host.size / float(np.median(v)) / 1e6
        line["results_only_over_match"] = line["results_only_ms"] / line["match_ms"]
        line["with_spans_over_match"] = line["with_spans_ms"] / line["match_ms"]
        line["found"] = int(res[2].sum())
        line["right"] = right
        text = json.dumps(line)
        print(text, flush=True)
        with open(OUT, "a") as f:
            f.write(text + "\n")
        img.close()


if __name__ == "__main__":
    main()
