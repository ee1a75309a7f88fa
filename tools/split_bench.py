#!/usr/bin/env python3
"""Text to batch on the device (mfa_split_text_count + mfa_split_text_write), measured two ways.  One JSON line per measurement, also
appended to profiles/r13_text_split.jsonl.

  split   count + write alone on SIZE bytes (default 1 GiB) of 1 KiB lines and of 8-byte tokens: device time from events around each
          call, median of REPS (default 20) after three uncounted rounds, in GB/s of TEXT (the two passes read the text twice and
          write it once; the write pass also writes one 8-byte offset per string)
  e2e     wall clock of `diploma -match-lines FILE` on a file of SIZE bytes of 1 KiB lines against the host paths on the same strings,
          same automaton (a|b)*abb: `diploma -match` (cin >> text, match_packed), `DIPLOMA_DEVICE_SPLIT=1 diploma -match`, and
          `diploma -match-file gt FILE` (getline, match_packed; it prints its time only); the host paths with the batch on one device
          (DIPLOMA_DEVICES=1), as the device path is

  split_bench.py [split|e2e|all] [SIZE_MiB] [REPS]
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "re2-modification_amd"))

import numpy as np

OUT = os.path.join(ROOT, "profiles", "r13_text_split.jsonl")
DIPLOMA = os.path.join(ROOT, "re2-modification_amd", "host", "diploma")


def report(line):
    text = json.dumps(line)
    print(text, flush=True)
    with open(OUT, "a") as f:
        f.write(text + "\n")


def text_of(kind, size, seed=1):
    """`size` bytes: lines of 1023 letters of {a, b} and a newline, or tokens of 8 letters and a blank"""
    period = 1024 if kind == "lines" else 9
    rng = np.random.default_rng(seed)
    text = rng.integers(97, 99, size=size // period * period, dtype=np.uint8).reshape(-1, period)
    text[:, -1] = 10 if kind == "lines" else 32
    return text.reshape(-1)


def bench_split(size, reps):
    import torch
    from mfa_amd import capi
    for kind, mode in (("lines", capi.SPLIT_LINES), ("tokens", capi.SPLIT_TOKENS)):
        host = text_of(kind, size)
        n_text = host.size
        d_text = torch.zeros((n_text + 15) // 16 * 16, dtype=torch.uint8, device="cuda")
        d_text[:n_text] = torch.from_numpy(host)
        work = torch.empty(capi.split_workspace_bytes(n_text), dtype=torch.uint8, device="cuda")
        d_info = torch.zeros(4, dtype=torch.int64, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        stop = b"exit" if kind == "tokens" else None
        capi.split_text_count(d_text.data_ptr(), n_text, mode, stop, work.data_ptr(), d_info.data_ptr(), 0, s)
        n, n_bytes = [int(x) for x in d_info.cpu()[:2]]
        d_bytes = torch.empty((n_bytes + 15) // 16 * 16, dtype=torch.uint8, device="cuda")
        d_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        count_ms, write_ms = [], []
        for r in range(reps + 3):
            ev[0].record()
            capi.split_text_count(d_text.data_ptr(), n_text, mode, stop, work.data_ptr(), d_info.data_ptr(), 0, s)
            ev[1].record()
            capi.split_text_write(d_text.data_ptr(), n_text, mode, work.data_ptr(), d_info.data_ptr(), d_bytes.data_ptr(), d_bytes.numel(),
                                  d_off.data_ptr(), n, 0, s)
            ev[2].record()
            torch.cuda.synchronize()
            if r >= 3:
                count_ms.append(ev[0].elapsed_time(ev[1]))
                write_ms.append(ev[1].elapsed_time(ev[2]))
        rest = [int(x) for x in d_info.cpu()]
        period = 1024 if kind == "lines" else 9
        right = (n == n_text // period and n_bytes == n * (period - 1) and rest[2] == period - 1 and rest[3] == 0
                 and bool(torch.equal(d_off[:1000].cpu(), torch.arange(1000, dtype=torch.int64) * (period - 1))))
        c, w = float(np.median(count_ms)), float(np.median(write_ms))
        report({"what": "split alone, %s" % kind, "device": torch.cuda.get_device_name(0), "text_bytes": n_text, "strings": n,
                "count_ms": c, "write_ms": w, "count_spread_ms": max(count_ms) - min(count_ms), "write_spread_ms": max(write_ms) - min(write_ms),
                "count_GB/s": n_text / c / 1e6, "write_GB/s": n_text / w / 1e6, "both_GB/s": n_text / (c + w) / 1e6, "reps": reps, "right": right})
        del d_text, d_bytes, d_off, work


def wall(args, stdin_path, env):
    t0 = time.perf_counter()
    with open(stdin_path, "rb") as f, open(os.devnull, "wb") as null:      # (cwd: -match-file leaves its drawings and results.txt there)
        subprocess.run([DIPLOMA] + args, stdin=f, stdout=null, stderr=null, env=env, check=True, cwd=os.path.dirname(stdin_path))
    return time.perf_counter() - t0


def bench_e2e(size):
    folder = tempfile.mkdtemp(prefix="split_bench_")
    try:
        text = text_of("lines", size)
        path, regex_in, match_in = (os.path.join(folder, n) for n in ("lines.txt", "regex.txt", "match_stdin.txt"))
        text.tofile(path)
        with open(regex_in, "wb") as f:
            f.write(b"(a|b)*abb\n")
        with open(match_in, "wb") as f:
            f.write(b"(a|b)*abb\n")
            text.tofile(f)
            f.write(b"exit\n")
        env = dict(os.environ, DIPLOMA_DEVICES="1")
        env.pop("DIPLOMA_DEVICE_SPLIT", None)
        runs = {"-match-lines FILE (device split)": lambda: wall(["-match-lines", path], regex_in, env),
                "DIPLOMA_DEVICE_SPLIT=1 -match (device split)": lambda: wall(["-match"], match_in, dict(env, DIPLOMA_DEVICE_SPLIT="1")),
                "-match (cin >> text, match_packed)": lambda: wall(["-match"], match_in, env),
                "-match-file gt FILE (getline, match_packed)": lambda: wall(["-match-file", "gt", path], regex_in, env)}
        out = {"what": "end to end, wall clock, 1 KiB lines", "text_bytes": int(text.size), "seconds": {}}
        for name, run in runs.items():
            run()                                               # once uncounted: the page cache, the first use of the device
            out["seconds"][name] = sorted(run() for _ in range(3))[1]
        report(out)
    finally:
        shutil.rmtree(folder, ignore_errors=True)


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    size = (int(sys.argv[2]) if len(sys.argv) > 2 else 1024) << 20
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    if what in ("split", "all"):
        bench_split(size, reps)
    if what in ("e2e", "all"):
        bench_e2e(size)


if __name__ == "__main__":
    main()
