#!/usr/bin/env python3
"""Opening polynomials over Fr at a point (mi_fr_poly_open, mi_fr_poly_open_device) on one MI355X: ONE JSON line, also written to
profiles/poly_bench.json.

    python tools/bench_poly.py                          n = 2^20, 2^24, 2^26 (one polynomial) and 64 polynomials of 2^12
    python tools/bench_poly.py --sizes 20:1,12:64       other (log2 n : batch) pairs
    python tools/bench_poly.py --no-cpu                 without the CPU baseline
    python tools/bench_poly.py --no-host-form

Per size two operations, `open` (quotient + value, in place) and `evaluate` (value only), each in the device form (coefficients stay in HBM) and
in the host form.  Per figure: warm-up, then at least 20 calls and 0.5 s; the median and the spread (minimum, maximum) over the calls.  `kernels_ms`
is mi_profile.accumulate_ms: HIP events on the library's stream around the sweeps of one call.  `hbm_gb_per_s` is the bytes the design moves (96 B
per element for an opening: two reads and one write; 32 B for an evaluation) over the kernels' time, `hbm_share` that against the 8.0 TB/s peak of
HBM3E.  `ntt_kernels_ms` is mi_fr_ntt_device on the same vectors in the same process, the two calls alternated.  `cpu_baseline` is
tests/host/fr_poly_ref.cpp (a serial Horner per polynomial) on 16 polynomials over 16 threads of the same machine, measured at n <= 2^20 (the
recurrence is linear in n: larger rows carry the rate measured at 2^20, marked as such).  After the timed calls one sparse polynomial is opened
and rows of the quotient are compared with the closed form."""
from __future__ import annotations

import argparse
import json
import os
import random
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GB_S = 8000.0


def timed(fn, min_calls=20, min_s=0.5):
    """-> wall seconds of every call"""
    out, t_all = [], time.perf_counter()
    while len(out) < min_calls or time.perf_counter() - t_all < min_s:
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def spread(xs, scale=1.0, digits=4):
    return {"median": round(statistics.median(xs) * scale, digits), "min": round(min(xs) * scale, digits), "max": round(max(xs) * scale, digits), "calls": len(xs)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20:1,24:1,26:1,12:64")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-host-form", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poly_bench.json"))
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_poly.py needs an MI355X: there is no CPU path to time")
    import numpy as np

    import __graft_entry__ as ge
    import poly_util as pu

    pkg = ge.load_package()
    rows = []
    ref_exe = None if args.no_cpu else pu.host_exe("fr_poly_ref")
    cpu_rate = {}   # evaluate_only -> elements/s at the largest n measured
    rnd = random.Random(0xBE)
    with pkg.Context([0]) as ctx:
        for item in args.sizes.split(","):
            log_n, batch = (int(x) for x in item.split(":"))
            n, total = 1 << log_n, batch << log_n
            w = np.random.default_rng(log_n).integers(0, 1 << 32, size=(total, 8), dtype=np.uint64).astype(np.uint32)
            w[:, 7] &= 0x3FFFFFFF
            d_src = torch.from_numpy(w.view(np.int32)).cuda()
            d_work = torch.empty_like(d_src)
            d_ntt = torch.empty_like(d_src)
            torch.cuda.synchronize()
            point = pu.pack([rnd.randrange(2, pu.R)], 1)
            for op in ("open", "evaluate"):
                # an opening runs in place on a buffer whose content no longer matters after the first call (the time does not depend on the values)
                d_q = d_work.data_ptr() if op == "open" else None
                dev = lambda: ctx.fr_poly_open_device(d_work.data_ptr(), n, batch, point, 1, d_q)
                ntt = lambda: ctx.fr_ntt_device(d_src.data_ptr(), log_n, batch, False, None, 1, d_ntt.data_ptr())
                d_work.copy_(d_src)
                torch.cuda.synchronize()
                for _ in range(3):
                    dev()
                    ntt()
                k_ms, ntt_ms = [], []
                def pair():
                    dev()
                    k_ms.append(ctx.profile()["accumulate_ms"])
                    ntt()
                    ntt_ms.append(ctx.profile()["accumulate_ms"])
                timed(pair)
                wall = timed(dev)
                dev()
                p = ctx.profile()
                bytes_moved = (96 if op == "open" else 32) * total
                km = statistics.median(k_ms)
                row = {"op": op, "log_n": log_n, "batch": batch, "levels": p["num_windows"], "tile_bits": p["window_bits"],
                       "device_ms": spread(wall, 1e3), "device_elements_per_s": total / statistics.median(wall),
                       "kernels_ms": spread(k_ms), "bytes_moved": bytes_moved, "hbm_gb_per_s": round(bytes_moved / (km * 1e-3) / 1e9, 1),
                       "hbm_share": round(bytes_moved / (km * 1e-3) / 1e9 / HBM_PEAK_GB_S, 4),
                       "ntt_kernels_ms": spread(ntt_ms), "kernels_vs_ntt": round(km / statistics.median(ntt_ms), 4)}
                if not args.no_host_form:
                    data = w.tobytes()
                    into = np.zeros(len(data), dtype=np.uint8) if op == "open" else None
                    host = lambda: ctx.fr_poly_open(data, n, batch, point, 1, quotients=op == "open", into=into)
                    host()
                    row["host_ms"] = spread(timed(host), 1e3)
                    del data, into
                if ref_exe and log_n <= 20:   # 16 polynomials, one per thread (larger sizes: the files alone are gigabytes)
                    cb = 16
                    cw = np.random.default_rng(1).integers(0, 1 << 32, size=(cb << log_n, 8), dtype=np.uint64).astype(np.uint32)
                    with tempfile.TemporaryDirectory() as tmp:
                        _, _, secs = pu.run_ref(ref_exe, tmp, cw.tobytes(), n, cb, point, 1, threads=16, evaluate_only=op == "evaluate")
                    del cw
                    rate = (cb << log_n) / secs
                    row["cpu_baseline"] = {"what": "tests/host/fr_poly_ref.cpp, 16 polynomials on 16 threads, same machine", "n": n, "s": round(secs, 4),
                                           "elements_per_s": rate}
                    cpu_rate[op] = (n, rate)
                elif ref_exe and op in cpu_rate:
                    row["cpu_baseline"] = {"what": "the rate measured at n = %d (the serial recurrence is linear in n), not measured at this size" % cpu_rate[op][0],
                                           "elements_per_s": cpu_rate[op][1]}
                if "cpu_baseline" in row:
                    row["device_vs_cpu"] = round(row["device_elements_per_s"] / row["cpu_baseline"]["elements_per_s"], 2)
                rows.append(row)
            # the last word: a sparse polynomial through the same call, rows against the closed form
            entries = {j % n: rnd.randrange(1, pu.R) for j in (0, 1, n // 2 + 1, n - 1, rnd.randrange(n))}
            z = pu.value_of_raw(pu.unpack_raw(point)[0], 1)
            d_work.zero_()
            for j, v in entries.items():
                d_work[j] = torch.frombuffer(bytearray(pu.pack([v], 1)), dtype=torch.int32).cuda()
            torch.cuda.synchronize()
            value = ctx.fr_poly_open_device(d_work.data_ptr(), n, 1, point, 1, d_work.data_ptr())
            pick = sorted({0, 1 % n, n // 2, n - 2, n - 1} | {rnd.randrange(n) for _ in range(256)})
            got = d_work[torch.tensor(pick, device="cuda")].cpu().numpy().tobytes()
            exact = got == pu.expected_bytes(pu.sparse_rows(entries, n, z, pick), 1) and value == pu.expected_bytes([pu.sparse_value(entries, z)], 1)
            for row in rows[-2:]:
                row["sparse_rows_exact"] = exact
            del d_src, d_work, d_ntt, w
            torch.cuda.empty_cache()
    out = {"metric": "opening polynomials over Fr at a point (quotient by X - z and value), Montgomery form", "unit": "elements/s",
           "hbm_peak_gb_per_s": HBM_PEAK_GB_S, "sizes": rows}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
