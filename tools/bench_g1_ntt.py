#!/usr/bin/env python3
"""Radix-2 NTT over G1 points (mi_g1_ntt_device) on one MI355X: ONE JSON line, also written to profiles/g1_ntt_bench.json.

    python tools/bench_g1_ntt.py                      2^12, 2^16, 2^20, both directions
    python tools/bench_g1_ntt.py --sizes 12,16        other sizes
    python tools/bench_g1_ntt.py --no-cpu             without the CPU baseline

Per size and direction: time of the device form (points stay in HBM, out of place), butterflies/s, the share of the call taken by the
normalisation and by the table build of the first call, and the implied Fp-multiplication rate — from the kernel's own model, counted here:
255 doublings at 6.8, one complete addition at 12 per non-zero digit of the non-adjacent form (a third of 255 on average), the two
additions of the butterfly — as a fraction of the accumulate kernel's, which the same process measures (the device-resident G1 MSM of 2^20
scalars: mi_profile.accumulate_adds mixed additions of 10 multiplications in accumulate_ms).  The input is a powers-of-tau SRS, so after the
timed calls sampled rows are compared with the closed form.  `cpu_baseline` is tests/host/g1_ntt_ref.c — the same transform over the C
oracle's point arithmetic — on 16 threads of the same machine at 2^14 points.  Warm-up, then at least 3 calls and 0.5 s per figure."""
from __future__ import annotations

import argparse
import json
import os
import random
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DBL_MULS, ADD_MULS, MADD_MULS = 6.8, 12.0, 10.0
CPU_LOG_N = 14


def timed(fn, min_calls=3, min_s=0.5):
    calls, t0 = 0, time.perf_counter()
    while calls < min_calls or time.perf_counter() - t0 < min_s:
        fn()
        calls += 1
    return (time.perf_counter() - t0) / calls, calls


def fp_muls(log_n: int, inverse: bool) -> float:
    """Fp multiplications of one transform by the model above: every butterfly adds twice, every butterfly with a twiddle other than 1
    (all but 2^l of level l, none of the last level) walks a 255-bit scalar; the inverse direction walks log_n + 1 more (butterfly
    (q = 0, p = 0) of every level and the extra lane of the last launch, which also adds once)"""
    n = 1 << log_n
    ladders = sum(n // 2 - (1 << level) for level in range(log_n - 1)) + (log_n + 1 if inverse else 0)
    return ladders * (255 * DBL_MULS + 255 / 3 * ADD_MULS) + ((n // 2) * log_n * 2 + (1 if inverse else 0)) * ADD_MULS


def accumulate_rate(pkg, co, torch):
    """Fp multiplications per second of the accumulate kernel: the device-resident G1 MSM of 2^20 scalars"""
    n = 1 << 20
    bases = co.gen_bases("g1", 0x7A1, n, 16)
    sc = co.gen_scalars(0x7A2, n, True)
    with pkg.Context([0]) as c:
        c.set_bases("g1", bases, n)
        d = torch.frombuffer(bytearray(sc), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        for _ in range(5):
            c.msm_device("g1", d.data_ptr(), n, 1)
        rates = []
        def one():
            c.msm_device("g1", d.data_ptr(), n, 1)
            p = c.profile()
            rates.append(p["accumulate_adds"] * MADD_MULS / (p["accumulate_ms"] * 1e-3))
        timed(one, min_calls=20)
    return sum(rates) / len(rates)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="12,16,20")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "g1_ntt_bench.json"))
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_g1_ntt.py needs an MI355X: there is no CPU path to time")
    import __graft_entry__ as ge
    import g1_ntt_util as gu
    from oracle import coracle as co

    pkg = ge.load_package()
    acc_rate = accumulate_rate(pkg, co, torch)
    gen = co.mul_gen("g1", 1)
    tau = random.Random(0x7A0).randrange(2, gu.R)
    rows = []
    cpu = None
    with pkg.Context([0]) as ctx:
        sizes = [int(x) for x in args.sizes.split(",")]
        for log_n in sizes + ([] if args.no_cpu or CPU_LOG_N in sizes else [CPU_LOG_N]):
            n = 1 << log_n
            d_pw = torch.frombuffer(bytearray(gu.pack_scalars(gu.powers(tau, n))), dtype=torch.uint8).cuda()
            d_in = torch.empty(gu.AFF * n, dtype=torch.uint8, device="cuda")
            d_out = torch.empty_like(d_in)
            torch.cuda.synchronize()
            ctx.batch_mul_device("g1", gen, d_pw.data_ptr(), n, 0, d_in.data_ptr())
            for inverse in (False, True):
                dev = lambda: ctx.g1_ntt_device(d_in.data_ptr(), log_n, inverse, d_out.data_ptr())
                t0 = time.perf_counter()
                dev()
                first_s = time.perf_counter() - t0
                build_ms = ctx.profile()["ingest_ms"]
                prof = []
                def dev_p():
                    dev()
                    prof.append(ctx.profile())
                dev_s, calls = timed(dev_p)
                k_ms = sum(p["accumulate_ms"] for p in prof) / len(prof)
                norm_ms = sum(p["reduce_ms"] for p in prof) / len(prof)
                rate = fp_muls(log_n, inverse) / (k_ms * 1e-3)
                rnd = random.Random(log_n)
                pick = sorted({0, 1, n // 2, n - 1} | {rnd.randrange(n) for _ in range(28)})
                sc = gu.closed_form_scalars(tau, log_n, inverse)
                got = d_out.view(n, gu.AFF)[torch.tensor(pick, device="cuda")].cpu().numpy().tobytes()
                row = {"log_n": log_n, "inverse": inverse, "levels": prof[-1]["num_windows"], "first_call_ms": round(first_s * 1e3, 3),
                       "table_build_ms": round(build_ms, 3), "table_build_share_of_first_call": build_ms / (first_s * 1e3),
                       "device_ms": round(dev_s * 1e3, 4), "device_calls": calls, "butterflies_per_s": (n // 2) * log_n / dev_s,
                       "level_kernels_ms": round(k_ms, 4), "normalise_ms": round(norm_ms, 4), "normalise_share": norm_ms / (dev_s * 1e3),
                       "fp_muls_model": fp_muls(log_n, inverse), "fp_muls_per_s": rate, "fraction_of_accumulate_rate": rate / acc_rate,
                       "sampled_rows_exact": got == b"".join(co.mul_gen("g1", sc[k]) for k in pick)}
                if log_n == CPU_LOG_N and not args.no_cpu and not inverse:
                    with tempfile.TemporaryDirectory() as tmp:
                        jac, secs = gu.run_ref(gu.ref_exe(), tmp, d_in.cpu().numpy().tobytes(), log_n, False, threads=16)
                    same = all(co.to_affine("g1", jac[gu.JAC * k:gu.JAC * (k + 1)]) == co.mul_gen("g1", sc[k]) for k in pick)
                    cpu = {"what": "tests/host/g1_ntt_ref.c, forward, 16 threads, same machine", "log_n": log_n, "s": round(secs, 4),
                           "butterflies_per_s": (n // 2) * log_n / secs, "sampled_rows_exact": same, "device_vs_cpu": secs / dev_s}
                rows.append(row)
            del d_pw, d_in, d_out
            torch.cuda.empty_cache()
    out = {"metric": "radix-2 NTT over G1 points, device form", "unit": "butterflies/s", "sizes": rows,
           "accumulate_kernel_fp_muls_per_s": acc_rate, "cpu_baseline": cpu}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
