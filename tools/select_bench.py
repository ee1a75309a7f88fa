#!/usr/bin/env python3
"""Batch to text on the device (mfa_select_count + mfa_select_write), measured two ways.  One JSON line per measurement, also appended
to profiles/r14_select.jsonl.

  select  count and write alone on the batch that the splitter makes of SIZE bytes (default 1 GiB) of 1 KiB lines and of 8-byte tokens,
          with all strings kept, every second and 1 in 100, MFA_SELECT_NEWLINE: device time from events around each call, median of REPS
          (default 20) after three uncounted rounds, in GB/s of OUTPUT; place_only_ms is the write call with no d_out_bytes (offsets and
          indices only), so write_ms - place_only_ms is the gather pass.  The yardstick, measured in the same run on the same text:
          mfa_split_text_write, the other call that moves every byte in and out through LDS
  e2e     wall clock of `diploma -grep-lines FILE` on a file of SIZE bytes of 1 KiB lines, automaton (a|b)*abb, output to a file,
          against the same binary with DIPLOMA_DEVICE_SELECT=0 (the selection on the host), with all lines kept and with 1 in 100;
          median of three runs after one uncounted

  select_bench.py [select|e2e|all] [SIZE_MiB] [REPS]
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

OUT = os.path.join(ROOT, "profiles", "r14_select.jsonl")
DIPLOMA = os.path.join(ROOT, "re2-modification_amd", "host", "diploma")
KEEP = (("all", 1), ("every second", 2), ("1 in 100", 100))


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


def median_ms(times):
    return float(np.median(times)), float(max(times) - min(times))


def bench_select(size, reps):
    import torch
    from mfa_amd import capi
    for kind, mode in (("lines", capi.SPLIT_LINES), ("tokens", capi.SPLIT_TOKENS)):
        period = 1024 if kind == "lines" else 9
        host = text_of(kind, size)
        n_text = host.size
        d_text = torch.zeros((n_text + 15) // 16 * 16, dtype=torch.uint8, device="cuda")
        d_text[:n_text] = torch.from_numpy(host)
        del host
        s = torch.cuda.current_stream().cuda_stream
        work = torch.empty(capi.split_workspace_bytes(n_text), dtype=torch.uint8, device="cuda")
        d_info = torch.zeros(4, dtype=torch.int64, device="cuda")
        capi.split_text_count(d_text.data_ptr(), n_text, mode, None, work.data_ptr(), d_info.data_ptr(), 0, s)
        n, n_bytes = [int(x) for x in d_info.cpu()[:2]]
        d_bytes = torch.empty((n_bytes + 15) // 16 * 16, dtype=torch.uint8, device="cuda")
        d_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        # the yardstick: the splitter's write call on this text, in this run
        yard = []
        for r in range(reps + 3):
            ev[0].record()
            capi.split_text_write(d_text.data_ptr(), n_text, mode, work.data_ptr(), d_info.data_ptr(), d_bytes.data_ptr(), d_bytes.numel(), d_off.data_ptr(), n, 0, s)
            ev[1].record()
            torch.cuda.synchronize()
            if r >= 3:
                yard.append(ev[0].elapsed_time(ev[1]))
        yard_ms, yard_spread = median_ms(yard)
        assert n == n_text // period and n_bytes == n * (period - 1)
        del d_text, work
        sel_work = torch.empty(capi.select_workspace_bytes(n), dtype=torch.uint8, device="cuda")
        sel_info = torch.zeros(4, dtype=torch.int64, device="cuda")
        flags = capi.SELECT_NEWLINE
        for name, every in KEEP:
            d_res = torch.zeros(n, dtype=torch.uint8, device="cuda")
            d_res[::every] = 1
            n_sel = (n + every - 1) // every
            out_bytes_n = n_sel * period
            out = torch.empty((out_bytes_n + 15) // 16 * 16, dtype=torch.uint8, device="cuda")
            out_off = torch.empty(n_sel + 1, dtype=torch.int64, device="cuda")
            out_ind = torch.empty(n_sel, dtype=torch.int64, device="cuda")
            count_ms, write_ms = [], []
            for r in range(reps + 3):
                ev[0].record()
                capi.select_count(d_res.data_ptr(), d_off.data_ptr(), n, flags, sel_work.data_ptr(), sel_info.data_ptr(), 0, s)
                ev[1].record()
                capi.select_write(d_bytes.data_ptr(), d_off.data_ptr(), d_res.data_ptr(), n, flags, sel_work.data_ptr(), sel_info.data_ptr(), out.data_ptr(),
                                  out_bytes_n, out_off.data_ptr(), out_ind.data_ptr(), n_sel, 0, s)
                ev[2].record()
                torch.cuda.synchronize()
                if r >= 3:
                    count_ms.append(ev[0].elapsed_time(ev[1]))
                    write_ms.append(ev[1].elapsed_time(ev[2]))
            # the write call without d_out_bytes (offsets and indices only): its place pass alone; what is left of write_ms is the gather pass
            place_ms = []
            for r in range(reps + 3):
                ev[0].record()
                capi.select_write(d_bytes.data_ptr(), d_off.data_ptr(), d_res.data_ptr(), n, flags, sel_work.data_ptr(), sel_info.data_ptr(), None, 0,
                                  out_off.data_ptr(), out_ind.data_ptr(), n_sel, 0, s)
                ev[1].record()
                torch.cuda.synchronize()
                if r >= 3:
                    place_ms.append(ev[0].elapsed_time(ev[1]))
            capi.select_write(d_bytes.data_ptr(), d_off.data_ptr(), d_res.data_ptr(), n, flags, sel_work.data_ptr(), sel_info.data_ptr(), out.data_ptr(),
                              out_bytes_n, out_off.data_ptr(), out_ind.data_ptr(), n_sel, 0, s)
            torch.cuda.synchronize()
            rest = [int(x) for x in sel_info.cpu()]
            first = min(1000, n_sel)
            right = (rest[0] == n_sel and rest[1] == out_bytes_n and rest[2] == 0 and rest[3] == 0
                     and bool(torch.equal(out_off[:first].cpu(), torch.arange(first, dtype=torch.int64) * period))
                     and bool(torch.equal(out_ind[:first].cpu(), torch.arange(first, dtype=torch.int64) * every))
                     and bool(torch.equal(out[:period - 1], d_bytes[:period - 1])) and int(out[period - 1]) == 10
                     and bool(torch.equal(out[out_bytes_n - period:out_bytes_n - 1], d_bytes[(n_sel - 1) * every * (period - 1):((n_sel - 1) * every + 1) * (period - 1)])))
            c, c_spread = median_ms(count_ms)
            w, w_spread = median_ms(write_ms)
            report({"what": "select alone, %s, %s kept" % (kind, name), "device": torch.cuda.get_device_name(0), "batch_bytes": n_bytes, "strings": n,
                    "selected": n_sel, "out_bytes": out_bytes_n, "count_ms": c, "write_ms": w, "both_ms": c + w, "place_only_ms": median_ms(place_ms)[0], "count_spread_ms": c_spread,
                    "write_spread_ms": w_spread, "write_out_GB/s": out_bytes_n / w / 1e6, "split_write_ms": yard_ms, "split_write_spread_ms": yard_spread,
                    "write_over_split_write": w / yard_ms, "reps": reps, "right": right})
            del d_res, out, out_off, out_ind
        del d_bytes, d_off, sel_work


def wall(args, stdin_path, out_path, env):
    t0 = time.perf_counter()
    with open(stdin_path, "rb") as f, open(out_path, "wb") as out, open(os.devnull, "wb") as null:
        subprocess.run([DIPLOMA] + args, stdin=f, stdout=out, stderr=null, env=env, check=True, cwd=os.path.dirname(stdin_path))
    return time.perf_counter() - t0


def bench_e2e(size):
    folder = tempfile.mkdtemp(prefix="select_bench_")
    try:
        path, regex_in, out_path = (os.path.join(folder, n) for n in ("lines.txt", "regex.txt", "kept.txt"))
        with open(regex_in, "wb") as f:
            f.write(b"(a|b)*abb\n")
        env = dict(os.environ, DIPLOMA_DEVICES="1")
        env.pop("DIPLOMA_DEVICE_SELECT", None)
        for name, every in (("all", 1), ("1 in 100", 100)):
            text = text_of("lines", size).reshape(-1, 1024)
            text[:, -4:-1] = (97, 97, 97)                      # no line matches ...
            text[::every, -4:-1] = (97, 98, 98)                # ... but these
            text.reshape(-1).tofile(path)
            want = (text.shape[0] + every - 1) // every * 1024
            del text
            out = {"what": "end to end, wall clock, 1 KiB lines, %s kept" % name, "text_bytes": os.path.getsize(path), "kept_bytes": want, "seconds": {}}
            for label, e in (("-grep-lines FILE (device select)", env), ("DIPLOMA_DEVICE_SELECT=0 -grep-lines FILE (host select)", dict(env, DIPLOMA_DEVICE_SELECT="0"))):
                wall(["-grep-lines", path], regex_in, out_path, e)      # once uncounted: the page cache, the first use of the device
                out["seconds"][label] = sorted(wall(["-grep-lines", path], regex_in, out_path, e) for _ in range(3))[1]
                with open(out_path, "rb") as f:                 # the few header lines of compile(), then the kept lines and nothing else
                    f.seek(max(os.path.getsize(out_path) - 1024, 0))
                    tail = f.read()
                out["right"] = (out.get("right", True) and 0 <= os.path.getsize(out_path) - want < 1024 and len(tail) == 1024
                                and tail.endswith(b"abb\n") and tail.count(b"\n") == 1)
            report(out)
    finally:
        shutil.rmtree(folder, ignore_errors=True)


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    size = (int(sys.argv[2]) if len(sys.argv) > 2 else 1024) << 20
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    if what in ("select", "all"):
        bench_select(size, reps)
    if what in ("e2e", "all"):
        bench_e2e(size)


if __name__ == "__main__":
    main()
