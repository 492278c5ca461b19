#!/usr/bin/env python3
"""Batched inversion and running products over Fr (mi_fr_batch_inverse, mi_fr_scan and their device forms) on one MI355X: ONE JSON line, also
written to profiles/scan_bench.json.

    python tools/bench_scan.py                          n = 2^20, 2^24, 2^26 (one vector) and 64 vectors of 2^12
    python tools/bench_scan.py --sizes 20:1,12:64       other (log2 n : batch) pairs
    python tools/bench_scan.py --no-cpu                 without the CPU baseline
    python tools/bench_scan.py --no-host-form

Per size four operations: `inverse`, `inverse_num` (with numerators), `scan` (the exclusive running product, in place) and `reduce` (the totals
alone), each in the device form (vectors stay in HBM) and in the host form.  The inversion has no batch: 64 vectors of 2^12 are one call of 2^18
elements for it.  Per figure: warm-up, then at least 20 calls and 0.5 s; the median and the spread (minimum, maximum) over the calls.  `kernels_ms`
is mi_profile.accumulate_ms: HIP events on the library's stream around the sweeps of one call.  `ntt_kernels_ms` is mi_fr_ntt_device on vectors
of the same size in the same process, the two calls alternated; `kernels_vs_ntt` the ratio of the medians.  `cpu_baseline` is
tests/host/fr_scan_ref.cpp on 16 threads of the same machine at n <= 2^20 (both operations are linear in n: larger rows carry the rate measured
at 2^20, marked as such).  `top_inversion` compares, at 2^12 elements, the inversion with the exclusive product scan: the same number of launches
and levels, so the difference bounds what the one inversion on one lane of the top level costs.  After the timed calls an almost constant vector
goes through the same calls and rows are compared with the closed forms."""
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

OPS = ("inverse", "inverse_num", "scan", "reduce")


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_bench.json"))
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_scan.py needs an MI355X: there is no CPU path to time")
    import numpy as np

    import __graft_entry__ as ge
    import scan_util as su

    pkg = ge.load_package()
    MUL = pkg.FR_MUL
    rows = []
    ref_exe = None if args.no_cpu else su.host_exe("fr_scan_ref")
    cpu_rate = {}   # op -> (n, elements/s) at the largest n measured
    rnd = random.Random(0xBE)

    def device_call(ctx, op, d_a, d_num, n, batch):
        total = n * batch
        if op == "inverse":
            return lambda: ctx.fr_batch_inverse_device(d_a.data_ptr(), None, total, 1, d_a.data_ptr())
        if op == "inverse_num":
            return lambda: ctx.fr_batch_inverse_device(d_a.data_ptr(), d_num.data_ptr(), total, 1, d_a.data_ptr())
        if op == "scan":
            return lambda: ctx.fr_scan_device(MUL, d_a.data_ptr(), n, batch, True, 1, d_a.data_ptr())
        return lambda: ctx.fr_scan_device(MUL, d_a.data_ptr(), n, batch, False, 1, None)

    def kernel_times(ctx, dev, ntt):
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
        return k_ms, ntt_ms

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
            ntt = lambda: ctx.fr_ntt_device(d_src.data_ptr(), log_n, batch, False, None, 1, d_ntt.data_ptr())
            for op in OPS:
                # in place on a buffer whose content no longer matters after the first call (the time does not depend on the values)
                dev = device_call(ctx, op, d_work, d_src, n, batch)
                d_work.copy_(d_src)
                torch.cuda.synchronize()
                k_ms, ntt_ms = kernel_times(ctx, dev, ntt)
                wall = timed(dev)
                dev()
                p = ctx.profile()
                km = statistics.median(k_ms)
                row = {"op": op, "log_n": log_n, "batch": batch, "levels": p["num_windows"], "tile_bits": p["window_bits"],
                       "device_ms": spread(wall, 1e3), "device_elements_per_s": total / statistics.median(wall), "kernels_ms": spread(k_ms),
                       "ntt_kernels_ms": spread(ntt_ms), "kernels_vs_ntt": round(km / statistics.median(ntt_ms), 4)}
                if not args.no_host_form:
                    data = w.tobytes()
                    into = np.zeros(len(data), dtype=np.uint8) if op != "reduce" else None
                    if op.startswith("inverse"):
                        host = lambda: ctx.fr_batch_inverse(data, data if op == "inverse_num" else None, 1, into=into)
                    else:
                        host = lambda: ctx.fr_scan(MUL, data, n, batch, True, 1, out=op == "scan", into=into)
                    host()
                    row["host_ms"] = spread(timed(host), 1e3)
                    del data, into
                if ref_exe and total <= 1 << 20:
                    with tempfile.TemporaryDirectory() as tmp:
                        blob = w.tobytes()
                        if op.startswith("inverse"):
                            secs = su.run_ref(ref_exe, tmp, "inverse", blob, total, 1, 1, 16, num=blob if op == "inverse_num" else None)[2]
                        else:
                            secs = su.run_ref(ref_exe, tmp, "scan", blob, n, batch, 1, 16, MUL, True, no_out=op == "reduce")[2]
                        del blob
                    row["cpu_baseline"] = {"what": "tests/host/fr_scan_ref.cpp on 16 threads, same machine", "n": total, "s": round(secs, 4),
                                           "elements_per_s": total / secs}
                    if batch == 1:
                        cpu_rate[op] = (total, total / secs)
                elif ref_exe and op in cpu_rate:
                    row["cpu_baseline"] = {"what": "the rate measured at n = %d (linear in n), not measured at this size" % cpu_rate[op][0],
                                           "elements_per_s": cpu_rate[op][1]}
                if "cpu_baseline" in row:
                    row["device_vs_cpu"] = round(row["device_elements_per_s"] / row["cpu_baseline"]["elements_per_s"], 2)
                rows.append(row)
                print("%s 2^%d x %d: kernels %.4f ms, %.3f of the NTT" % (op, log_n, batch, km, row["kernels_vs_ntt"]), file=sys.stderr, flush=True)
            # the last word: an almost constant vector through the same calls, rows against the closed forms
            c = rnd.randrange(2, su.R)
            specials = {j % total: rnd.randrange(1, su.R) for j in (0, 1, total // 2 + 1, total - 1, rnd.randrange(total))}
            pick = sorted({0, 1 % total, total // 2, total - 2, total - 1} | {rnd.randrange(total) for _ in range(256)})
            idx = torch.tensor(pick, device="cuda")

            def fill():
                d_work.copy_(torch.frombuffer(bytearray(su.pack([c], 1)), dtype=torch.int32).cuda().repeat(total, 1))
                for j, v in specials.items():
                    d_work[j] = torch.frombuffer(bytearray(su.pack([v], 1)), dtype=torch.int32).cuda()
                torch.cuda.synchronize()
            fill()
            zeros = ctx.fr_batch_inverse_device(d_work.data_ptr(), None, total, 1, d_work.data_ptr())
            exact = zeros == 0 and d_work[idx].cpu().numpy().tobytes() == su.expected_bytes(su.sparse_inverse_rows(c, specials, pick), 1)
            if batch == 1:
                fill()
                tot = ctx.fr_scan_device(MUL, d_work.data_ptr(), n, 1, True, 1, d_work.data_ptr())
                exact = exact and d_work[idx].cpu().numpy().tobytes() == su.expected_bytes(su.sparse_scan_rows(c, specials, MUL, True, pick), 1)
                exact = exact and tot == su.expected_bytes([su.sparse_scan_total(c, specials, MUL, n)], 1)
            for row in rows[-len(OPS):]:
                row["closed_form_rows_exact"] = exact
            del d_src, d_work, d_ntt, w
            torch.cuda.empty_cache()
        # the one inversion of a call: at 2^12 the inversion and the exclusive product scan run the same launches over the same levels
        n = 1 << 12
        w = np.random.default_rng(12).integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)
        w[:, 7] &= 0x3FFFFFFF
        d_src = torch.from_numpy(w.view(np.int32)).cuda()
        d_work, d_ntt = d_src.clone(), torch.empty_like(d_src)
        torch.cuda.synchronize()
        ntt = lambda: ctx.fr_ntt_device(d_src.data_ptr(), 12, 1, False, None, 1, d_ntt.data_ptr())
        inv_ms, ntt_ms = kernel_times(ctx, device_call(ctx, "inverse", d_work, d_src, n, 1), ntt)
        scan_ms, _ = kernel_times(ctx, device_call(ctx, "scan", d_work, d_src, n, 1), ntt)
        mi, ms = statistics.median(inv_ms), statistics.median(scan_ms)
        top = {"log_n": 12, "inverse_kernels_ms": spread(inv_ms), "scan_kernels_ms": spread(scan_ms), "ntt_kernels_ms": spread(ntt_ms),
               "difference_ms": round(mi - ms, 4), "share_of_inverse_at_most": round((mi - ms) / mi, 4)}
    out = {"metric": "batched inversion and running products over Fr, Montgomery form", "unit": "elements/s", "sizes": rows, "top_inversion": top}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
