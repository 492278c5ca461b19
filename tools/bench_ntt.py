#!/usr/bin/env python3
"""Radix-2 NTT over Fr (mi_fr_ntt, mi_fr_ntt_device) on one MI355X: ONE JSON line, also written to profiles/ntt_bench.json.

    python tools/bench_ntt.py                            2^16, 2^20, 2^24, 2^26 (device and host form) and batch = 64 at 2^12
    python tools/bench_ntt.py --sizes 20:1,12:64         other (log_n:batch) pairs
    python tools/bench_ntt.py --msm-lib PATH             the MSM yardstick also with another build of the library (a child process)
    python tools/bench_ntt.py --no-cpu                   without the CPU baseline

Per size: time and elements/s of the device form (vectors stay in HBM, out of place) and of the host form; the kernels' own time
(mi_profile.accumulate_ms); bytes moved per pass and in all passes against the kernels' time; Fr multiplications (butterflies + twiddle joins
+ format conversions, counted here from the pass plan) per second.  After the timed calls one sparse vector is transformed and rows of the
result are compared with the closed form.  `yardstick` is the project's own: the device-resident G1 MSM of 2^20 Montgomery scalars in the same
process.  `cpu_baseline` is tests/host/fr_ntt_ref.cpp on 16 threads of the same machine (the batch carries the parallelism: 16 vectors).
Warm-up, then at least 20 calls and 0.5 s per figure."""
from __future__ import annotations

import argparse
import json
import os
import random
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, min_calls=20, min_s=0.5):
    calls, t0 = 0, time.perf_counter()
    while calls < min_calls or time.perf_counter() - t0 < min_s:
        fn()
        calls += 1
    return (time.perf_counter() - t0) / calls, calls


def fr_muls(log_n: int, passes: int, fmt: int) -> int:
    """Fr multiplications of one forward transform of 2^log_n elements, from the plan of ntt_kernels.cuh: one per butterfly except at the last
    level, one more where the twiddle is joined from both tables, and the format conversions of canonical input and output"""
    n = 1 << log_n
    bits = max(log_n - 1, 0)
    h = (bits + 1) // 2
    total = 0
    for level in range(log_n):
        if level + 1 == log_n:
            continue
        total += (n // 2) * (2 if level < h and bits > h else 1)
    return total + (2 * n if fmt == 0 else 0)


def msm_yardstick(pkg, co, torch, lib=None):
    """seconds per device-resident G1 MSM of 2^20 Montgomery scalars (mi_msm_g1_device over resident bases)"""
    if lib:
        pkg.binding.lib_path = lambda test_hooks=False: lib
    n = 1 << 20
    bases = co.gen_bases("g1", 0x7A1, n, 16)
    sc = co.gen_scalars(0x7A2, n, True)
    with pkg.Context([0]) as c:
        c.set_bases("g1", bases, n)
        d = torch.frombuffer(bytearray(sc), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        for _ in range(5):
            c.msm_device("g1", d.data_ptr(), n, 1)
        s, calls = timed(lambda: c.msm_device("g1", d.data_ptr(), n, 1))
    return {"what": "mi_msm_g1_device, 2^20 resident bases, Montgomery scalars", "ms": round(s * 1e3, 4), "calls": calls,
            "library": os.path.relpath(lib or pkg.lib_path(), ROOT)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16:1,20:1,24:1,26:1,12:64")
    ap.add_argument("--msm-lib", default=None, help="another build of libarkblst_amd.so for the MSM yardstick (measured in a child process)")
    ap.add_argument("--msm-only", action="store_true", help="print the MSM yardstick of --lib and nothing else")
    ap.add_argument("--lib", default=None, help="another build of libarkblst_amd.so to measure instead of the tree's (A/B on one machine)")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-host-form", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ntt_bench.json"))
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_ntt.py needs an MI355X: there is no CPU path to time")
    import numpy as np

    import __graft_entry__ as ge
    import ntt_util as nu
    from oracle import coracle as co

    pkg = ge.load_package()
    if args.msm_only:
        print(json.dumps(msm_yardstick(pkg, co, torch, args.lib)))
        return
    if args.lib:
        pkg.binding.lib_path = lambda test_hooks=False: os.path.abspath(args.lib)
    rows = []
    ref_exe = None if args.no_cpu else nu.host_exe("fr_ntt_ref")
    with pkg.Context([0]) as ctx:
        for item in args.sizes.split(","):
            log_n, batch = (int(x) for x in item.split(":"))
            n, total = 1 << log_n, batch << log_n
            w = np.random.default_rng(log_n).integers(0, 1 << 32, size=(total, 8), dtype=np.uint64).astype(np.uint32)
            w[:, 7] &= 0x3FFFFFFF
            d_in = torch.from_numpy(w.view(np.int32)).cuda()
            d_out = torch.empty_like(d_in)
            torch.cuda.synchronize()
            dev = lambda: ctx.fr_ntt_device(d_in.data_ptr(), log_n, batch, False, None, 1, d_out.data_ptr())
            t0 = time.perf_counter()
            dev()
            first_s = time.perf_counter() - t0
            build_ms = ctx.profile()["ingest_ms"]
            for _ in range(3):
                dev()
            kms = []
            def dev_k():
                dev()
                kms.append(ctx.profile()["accumulate_ms"])
            dev_s, dev_calls = timed(dev_k)
            p = ctx.profile()
            k_ms = sum(kms) / len(kms)
            muls = fr_muls(log_n, p["num_windows"], 1) * batch
            row = {"log_n": log_n, "batch": batch, "passes": p["num_windows"], "levels_widest_pass": p["window_bits"],
                   "first_call_ms": round(first_s * 1e3, 3), "table_build_ms": round(build_ms, 3),
                   "device_ms": round(dev_s * 1e3, 4), "device_calls": dev_calls, "device_elements_per_s": total / dev_s,
                   "kernels_ms": round(k_ms, 4), "bytes_per_pass": 64 * total, "bytes_all_passes": 64 * total * p["num_windows"],
                   "hbm_gb_per_s": 64 * total * p["num_windows"] / (k_ms * 1e-3) / 1e9, "fr_muls": muls, "fr_muls_per_s": muls / (k_ms * 1e-3)}
            if not args.no_host_form:
                data = w.tobytes()
                into = np.zeros(len(data), dtype=np.uint8)
                host = lambda: ctx.fr_ntt(data, log_n, batch, False, None, 1, into=into)
                host()
                host_s, host_calls = timed(host)
                row.update({"host_ms": round(host_s * 1e3, 4), "host_calls": host_calls, "host_elements_per_s": total / host_s,
                            "host_equals_device": into.tobytes() == d_out.cpu().numpy().tobytes()})
                del data, into
            # the last word: a sparse vector through the same call, rows against the closed form
            rnd = random.Random(log_n)
            entries = {j % n: rnd.randrange(1, nu.R) for j in (0, 1, n // 2 + 1, n - 1, rnd.randrange(n))}
            d_in.zero_()
            for j, v in entries.items():
                d_in[j] = torch.frombuffer(bytearray(nu.pack([v], 1)), dtype=torch.int32).cuda()
            torch.cuda.synchronize()
            dev()
            pick = sorted({0, 1 % n, n // 2, n - 1} | {rnd.randrange(n) for _ in range(256)})
            got = d_out[torch.tensor(pick, device="cuda")].cpu().numpy().tobytes()
            row["sparse_rows_exact"] = got == nu.expected_bytes(nu.sparse_rows(entries, log_n, pick, False), 1)
            if ref_exe and log_n <= 20:   # 16 vectors, one per thread (larger sizes: the files alone are gigabytes)
                cb = 16
                cw = np.random.default_rng(1).integers(0, 1 << 32, size=(cb << log_n, 8), dtype=np.uint64).astype(np.uint32)
                with tempfile.TemporaryDirectory() as tmp:
                    _, secs = nu.run_ref(ref_exe, tmp, cw.tobytes(), log_n, cb, False, None, 1, threads=16)
                row["cpu_baseline"] = {"what": "tests/host/fr_ntt_ref.cpp, 16 vectors on 16 threads, same machine", "s": round(secs, 4),
                                       "elements_per_s": (cb << log_n) / secs}
                row["device_vs_cpu"] = (total / dev_s) / ((cb << log_n) / secs)
                del cw
            rows.append(row)
            del d_in, d_out, w
            torch.cuda.empty_cache()
    out = {"metric": "radix-2 NTT over Fr, forward, Montgomery form", "unit": "elements/s", "sizes": rows}
    out["yardstick"] = msm_yardstick(pkg, co, torch)
    if args.msm_lib:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--msm-only", "--lib", os.path.abspath(args.msm_lib)], capture_output=True, text=True, timeout=900)
        out["yardstick_other_build"] = json.loads(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 else {"error": r.stderr[-500:]}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
