"""Memory-less automata through mfa_match_mixed against the loop of per-image mfa_match_batch calls (the parent's code, unchanged).
  python tools/mixed_dfa.py [reps] [out.jsonl]          (default: 15 repetitions, profiles/r07_mixed_dfa.jsonl)
Corpora: (a) the 26 memory-less fixtures, 4 096 strings of up to 1 KiB each; (b) one memory-less automaton, 1 Mi x 1 KiB; and a sweep
of one segment's size between them (multi-table launch forced against a launch of its own) for the default of MFA_MIXED_DFA_OWN.
Both forms run alternately in one process, warm, timed with device events on one stream; min and median per form, and the loop's
run-to-run spread (max - min of its repetitions) as the yardstick."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "re2-modification_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import oracle_lib  # noqa: E402
from mfa_amd import capi, image  # noqa: E402
from testlib import NFA_NAMES  # noqa: E402


def corpus(n_seg, per_seg, max_len, rng, fixed=False):
    """n_seg segments of per_seg strings over {a, b}, lengths uniform in [0, max_len] (fixed: exactly max_len): device tensors"""
    n = n_seg * per_seg
    lens = np.full(n, max_len, dtype=np.int64) if fixed else rng.integers(0, max_len + 1, size=n).astype(np.int64)
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    g = torch.Generator(device="cuda")
    g.manual_seed(int(rng.integers(1 << 30)))
    d_bytes = (torch.randint(0, 2, (int(off[-1]) + 64,), generator=g, device="cuda", dtype=torch.uint8) + ord("a"))
    return d_bytes, torch.from_numpy(off).cuda(), off, [k * per_seg for k in range(n_seg + 1)]


def timed(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def ab(forms, reps, stream):
    """forms: name -> callable; alternately, after two warm-up rounds"""
    times = {k: [] for k in forms}
    for r in range(reps + 2):
        for k, fn in forms.items():
            ms = timed(fn, stream)
            if r >= 2:
                times[k].append(ms)
    return {k: {"min_ms": float(np.min(v)), "median_ms": float(np.median(v)), "max_ms": float(np.max(v))} for k, v in times.items()}


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r07_mixed_dfa.jsonl")
    names = NFA_NAMES
    images = [capi.Image(image.blob_from_dump(oracle_lib.load_dump(n))) for n in names]
    rng = np.random.default_rng(7)
    stream = torch.cuda.Stream()
    lines = []

    def run(tag, imgs, d_bytes, d_off, off, seg_first, env, extra=None):
        for k in ("MFA_MIXED_DFA", "MFA_MIXED_DFA_OWN", "MFA_MIXED_SINGLE_DIRECT"):
            os.environ.pop(k, None)
        os.environ.update(env)
        mixed = capi.Mixed(imgs)
        n = len(off) - 1
        res_m = torch.zeros(n, dtype=torch.uint8, device="cuda")
        res_l = torch.zeros(n, dtype=torch.uint8, device="cuda")
        total = int(off[-1])

        def one_mixed():
            mixed.match_tensors(d_bytes, d_off, seg_first, res_m, stream=stream, total_bytes=total)

        def loop():
            for k, im in enumerate(imgs):
                a, b = seg_first[k], seg_first[k + 1]
                if b > a:
                    im.match_tensors(d_bytes, d_off[a:b + 1], res_l[a:b], stream=stream)

        with torch.cuda.stream(stream):
            t = ab({"mixed": one_mixed, "loop": loop}, reps, stream)
        torch.cuda.synchronize()
        same = bool(torch.equal(res_m, res_l))
        line = {"case": tag, "images": len(imgs), "strings": n, "bytes": total, "env": env, "reps": reps, "mixed": t["mixed"], "loop": t["loop"],
                "loop_spread_ms": t["loop"]["max_ms"] - t["loop"]["min_ms"], "last_dfa": mixed.last_dfa(), "answers_equal": same}
        line["mixed_minus_loop_median_ms"] = t["mixed"]["median_ms"] - t["loop"]["median_ms"]
        line["within_spread"] = line["mixed_minus_loop_median_ms"] <= line["loop_spread_ms"]
        if extra:
            line.update(extra)
        print(json.dumps(line), flush=True)
        lines.append(line)
        mixed.close()

    # (a) many small segments
    d_bytes, d_off, off, sf = corpus(26, 4096, 1024, rng)
    run("a: 26 fixtures x 4096 strings of up to 1 KiB, MFA_MIXED_DFA=1 (one multi-table launch)", images, d_bytes, d_off, off, sf, {"MFA_MIXED_DFA": "1"})
    run("a: the same, MFA_MIXED_DFA=0 (26 launches inside the mixed call)", images, d_bytes, d_off, off, sf, {"MFA_MIXED_DFA": "0"})
    del d_bytes, d_off
    # the crossover: one segment of S strings x 1 KiB, in the multi-table launch against a launch of its own (both inside the mixed call:
    # MFA_MIXED_SINGLE_DIRECT=0 keeps the one-automaton call from turning into mfa_match_batch itself)
    one = [images[names.index("nfa_abb_thompson")]]
    for s in (4096, 16384, 32768, 65536, 262144, 1 << 20):
        d_bytes, d_off, off, sf = corpus(1, s, 1024, rng, fixed=True)
        run("sweep: 1 x %d strings x 1 KiB in the multi-table launch" % s, one, d_bytes, d_off, off, sf, {"MFA_MIXED_DFA": "1", "MFA_MIXED_SINGLE_DIRECT": "0", "MFA_MIXED_DFA_OWN": str(1 << 40)}, {"sweep": s, "form": "multi"})
        run("sweep: 1 x %d strings x 1 KiB in a launch of its own" % s, one, d_bytes, d_off, off, sf, {"MFA_MIXED_DFA": "1", "MFA_MIXED_SINGLE_DIRECT": "0", "MFA_MIXED_DFA_OWN": "1"}, {"sweep": s, "form": "own"})
        if s == 1 << 20:
            # (b) BASELINE configs[1] with the default knobs, alone and beside a second, small segment (so that the call is a real mixed one)
            run("b: 1 Mi x 1 KiB, one automaton, MFA_MIXED_DFA=1, default MFA_MIXED_DFA_OWN", one, d_bytes, d_off, off, sf, {"MFA_MIXED_DFA": "1"})
            two = [one[0], images[names.index("nfa_enum_glushkov")]]
            run("b: 1 Mi x 1 KiB, the last 4096 strings a second automaton's, MFA_MIXED_DFA=1, default MFA_MIXED_DFA_OWN", two, d_bytes, d_off, off, [0, s - 4096, s], {"MFA_MIXED_DFA": "1"})
        del d_bytes, d_off
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
