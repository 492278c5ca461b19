#!/usr/bin/env python3
"""Fixed-base batch multiplication out[i] = s_i * G (mi_g{1,2}_batch_mul, mi_g{1,2}_batch_mul_device) on one MI355X: ONE JSON line.

    python tools/bench_batch_mul.py                          G1 at 2^16, 2^20, 2^24 and G2 at 2^20
    python tools/bench_batch_mul.py --sizes g1:16,g2:16      other sizes
    python tools/bench_batch_mul.py --scan                   every w of {8, 10, 12, 13, 16} forced at n = 2^16 and 2^20 (profiles/fixed_base_w_scan.json)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_batch_mul.py --once
    python tools/bench_batch_mul.py --kernel-stats DIR       the same sizes, with the walk kernel's time taken from that separate run

Per size: points/s of the device form (scalars and points stay in HBM) and of the host form, the table build of a FIRST call apart from
the steady state, the walk kernel's mixed additions per second (n x non-zero digits, counted here from the scalars, over the kernel time
of the rocprofv3 run when --kernel-stats is given, over the library's own event time otherwise), and the oracle's gen_bases on 16 threads
of the same box as cpu_baseline.  The last result of every size is compared bit for bit with that oracle output.  `yardstick` is
k_accumulate<G1C> in the same process: accumulate_adds / accumulate_ms of a 2^20-point MSM, the figure bench.py --full reports — what a
mixed addition costs on this chip.  Warm-up, then at least 20 calls or 0.5 s per figure."""
from __future__ import annotations

import argparse
import csv
import ctypes as C
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 0xBA7C4


def windows(w: int) -> int:
    return (255 + w - 1) // w + (1 if 255 % w == 0 else 0)


def nonzero_digits(sc: bytes, w: int) -> int:
    """non-zero signed w-bit digits of all scalars (the recoding of fixed_base_kernels.cuh fb_digit, vectorised)"""
    import numpy as np

    a = np.frombuffer(sc, dtype="<u8").reshape(-1, 4)
    a = np.concatenate([a, np.zeros((a.shape[0], 1), dtype=np.uint64)], axis=1)
    carry = np.zeros(a.shape[0], dtype=np.uint64)
    half, full, total = np.uint64(1 << (w - 1)), np.uint64(1 << w), 0
    for j in range(windows(w)):
        off = w * j
        word, sh = off // 64, off % 64
        if word >= 4:
            v = np.zeros(a.shape[0], dtype=np.uint64)
        else:
            v = a[:, word] >> np.uint64(sh)
            if sh + w > 64:
                v = v | (a[:, word + 1] << np.uint64(64 - sh))
        raw = (v & (full - np.uint64(1))) + carry
        carry = (raw > half).astype(np.uint64)
        total += int(np.count_nonzero((raw != 0) & (raw != full)))
    return total


def timed(fn, min_calls=20, min_s=0.5):
    """mean seconds per call over at least min_calls calls and min_s seconds (fn ends in a device synchronise)"""
    calls, t0 = 0, time.perf_counter()
    while calls < min_calls or time.perf_counter() - t0 < min_s:
        fn()
        calls += 1
    return (time.perf_counter() - t0) / calls, calls


def walk_ms_from_stats(path: str):
    """{'g1': (calls, total ms), 'g2': ...} of the walk kernels from a rocprofv3 --kernel-trace --stats run (DIR or the csv itself)"""
    files = [path] if os.path.isfile(path) else sorted(glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True))
    out = {}
    for f in files:
        for row in csv.DictReader(open(f)):
            name = row.get("Name", "")
            for g, key in (("g1", "k_fb_walk<msmk::G1C>"), ("g2", "k_fb_walk_g2_coop")):
                if key in name:
                    c, ns = out.get(g, (0, 0.0))
                    out[g] = (c + int(row["Calls"]), ns + float(row["TotalDurationNs"]))
    return {g: (c, ns * 1e-6) for g, (c, ns) in out.items()}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="g1:16,g1:20,g1:24,g2:20")
    ap.add_argument("--scan", action="store_true", help="force w in {8, 10, 12, 13, 16} at n = 2^16 and 2^20, both groups; device form only")
    ap.add_argument("--once", action="store_true", help="one warm-up and 5 steady device-form calls per size and nothing else (for a profiler run)")
    ap.add_argument("--kernel-stats", default=None, metavar="DIR", help="kernel stats of a separate `rocprofv3 --kernel-trace --stats ... --once` run")
    ap.add_argument("--window-bits", type=int, default=0)
    ap.add_argument("--no-host-form", action="store_true")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_batch_mul.py needs an MI355X: there is no CPU path to time")
    import __graft_entry__ as ge
    from oracle import coracle as co

    pkg = ge.load_package()
    stats = walk_ms_from_stats(args.kernel_stats) if args.kernel_stats else {}
    sizes = [(s.split(":")[0], int(s.split(":")[1])) for s in args.sizes.split(",")]
    if args.scan:
        sizes = [(g, ln) for g in ("g1", "g2") for ln in (16, 20)]
    ONCE_CALLS = 5
    rows = []
    with pkg.Context([0]) as ctx:
        for group, ln in sizes:
            n = 1 << ln
            aff = 96 if group == "g1" else 192
            buf = C.create_string_buffer(32 * n)
            co.lib().orc_gen_dlogs(SEED + ln, n, buf)
            sc = buf.raw
            gen = co.mul_gen(group, 1)
            d_sc = torch.frombuffer(bytearray(sc), dtype=torch.uint8).cuda()
            d_out = torch.empty(n * aff, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            dev = lambda: ctx.batch_mul_device(group, gen, d_sc.data_ptr(), n, 0, d_out.data_ptr())
            if args.once:
                ctx.set_batch_mul_window_bits(args.window_bits)
                dev()
                w = ctx.profile()["window_bits"]
                for _ in range(ONCE_CALLS):
                    dev()
                rows.append({"group": group, "log_n": ln, "w": w, "device_calls": ONCE_CALLS + 1, "nonzero_digits": nonzero_digits(sc, w)})
                continue
            t0 = time.perf_counter()
            want = co.gen_bases(group, SEED + ln, n, 16)
            cpu_s = time.perf_counter() - t0
            for w_forced in ([8, 10, 12, 13, 16] if args.scan else [args.window_bits]):
                ctx.set_batch_mul_window_bits(w_forced)
                ctx.batch_mul(group, co.mul_gen(group, 3), sc[:32], 0)          # another base: the next call builds its table
                t0 = time.perf_counter()
                dev()
                first_s = time.perf_counter() - t0
                p = ctx.profile()
                w, build_ms = p["window_bits"], p["ingest_ms"]
                for _ in range(3):
                    dev()
                kms = []
                def dev_k():
                    dev()
                    kms.append(ctx.profile()["accumulate_ms"])
                dev_s, dev_calls = timed(dev_k)
                ok = d_out.cpu().numpy().tobytes() == want
                digits = nonzero_digits(sc, w)
                walk_ms, src = sum(kms) / len(kms), "library events (mi_profile.accumulate_ms)"
                row = {"group": group, "log_n": ln, "w": w, "num_windows": windows(w), "table_mib": round((windows(w) << (w - 1)) * (128 if group == "g1" else 256) / 2 ** 20, 2),
                       "first_call_ms": round(first_s * 1e3, 3), "table_build_ms": round(build_ms, 3),
                       "device_ms": round(dev_s * 1e3, 4), "device_points_per_s": n / dev_s, "device_calls": dev_calls,
                       "walk_kernel_ms": round(walk_ms, 4), "walk_kernel_ms_source": src, "nonzero_digits": digits,
                       "walk_adds_per_s": digits / (walk_ms * 1e-3), "cpu_baseline": {"what": "oracle gen_bases, 16 threads, same box", "s": round(cpu_s, 4),
                                                                                   "points_per_s": n / cpu_s},
                       "device_vs_cpu": cpu_s / dev_s, "bit_exact": ok}
                if not args.scan and not args.no_host_form:
                    import numpy as np

                    into = np.zeros(n * aff, dtype=np.uint8)
                    host = lambda: ctx.batch_mul(group, gen, sc, 0, into=into)
                    host()
                    host_s, host_calls = timed(host)
                    row.update({"host_ms": round(host_s * 1e3, 4), "host_points_per_s": n / host_s, "host_calls": host_calls,
                                "bit_exact": ok and into.tobytes() == want})
                rows.append(row)
            ctx.set_batch_mul_window_bits(0)
            del d_sc, d_out
        out = {"metric": "fixed-base batch_mul", "unit": "points/s", "sizes": rows}
        if args.once:
            out["note"] = "profiler leg: no timing taken here"
        else:
            # the yardstick: what a mixed addition costs in k_accumulate<G1C>, same process, same box
            n = 1 << 20
            bases = co.gen_bases("g1", SEED, n, 16)
            msc = co.gen_scalars(SEED + 1, n)
            ctx.set_bases("g1", bases, n)
            d_m = torch.frombuffer(bytearray(msc), dtype=torch.uint8).cuda()
            torch.cuda.synchronize()
            for _ in range(5):
                ctx.msm_device("g1", d_m.data_ptr(), n, 0)
            acc = []
            def msm_k():
                ctx.msm_device("g1", d_m.data_ptr(), n, 0)
                p = ctx.profile()
                acc.append((p["accumulate_adds"], p["accumulate_ms"]))
            timed(msm_k)
            adds, ms = sum(a for a, _ in acc) / len(acc), sum(m for _, m in acc) / len(acc)
            out["yardstick"] = {"kernel": "k_accumulate<G1C>, 2^20-point MSM", "accumulate_adds": adds, "accumulate_ms": round(ms, 4), "adds_per_s": adds / (ms * 1e-3)}
    if stats and not args.once:
        # kernel time of the separate rocprofv3 run (--once: 1 first + 5 steady calls per size): per group, total over the sizes of that run
        per_group = {}
        for r in rows:
            per_group.setdefault(r["group"], []).append(r)
        out["rocprof"] = {}
        for g, (calls, ms) in stats.items():
            rs = per_group.get(g, [])
            digits = sum(r["nonzero_digits"] * (ONCE_CALLS + 1) for r in rs)
            out["rocprof"][g] = {"walk_kernel_calls": calls, "walk_kernel_ms_total": round(ms, 4), "nonzero_digits_total": digits,
                                 "walk_adds_per_s": digits / (ms * 1e-3) if ms else None,
                                 "source": "rocprofv3 --kernel-trace --stats of a separate --once run over the same sizes (6 calls per size)"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
