"""CPU tests of the NTT over G1 points (mi_g1_ntt, mi_g1_ntt_device): the C ABI surface, the digit recoding of a twiddle and the level plan
with the butterfly body of csrc/g1_ntt_kernels.cuh compiled as plain C++ and run as a serial loop (also under AddressSanitizer + UBSan, as a
stand-alone program), and the resources of the kernel in the shipped code objects.  Points compare byte for byte against the definition
computed by the C oracle (tests/g1_ntt_util.py)."""
import ctypes as C
import os
import random
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import g1_ntt_util as gu  # noqa: E402
import ntt_util as nu  # noqa: E402

SYMS = ("mi_g1_ntt", "mi_g1_ntt_device")
R = gu.R


def test_symbols_declared_exported_and_bound(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "arkblst_amd.h")).read(), flags=re.S)
    for s in SYMS:
        assert re.search(r"\bint\s+%s\s*\(" % s, text), s
    for test_hooks in (False, True):
        exported = subprocess.check_output(["nm", "-D", "--defined-only", pkg.lib_path(test_hooks)]).decode()
        for s in SYMS:
            assert re.search(r" T %s$" % s, exported, flags=re.M), (s, test_hooks)
    L = pkg.load_library()
    vp, u, i = C.c_void_p, C.c_uint, C.c_int
    assert L.mi_g1_ntt.argtypes == [vp, vp, u, i, vp]
    assert L.mi_g1_ntt_device.argtypes == [vp, vp, u, i, vp]
    for name in ("g1_ntt", "g1_ntt_device"):
        assert callable(getattr(pkg.Context, name))
    # no context: MI_E_INVALID before anything is touched
    out = C.create_string_buffer(2 * gu.AFF)
    assert L.mi_g1_ntt(None, bytes(2 * gu.AFF), 1, 0, out) == -1
    assert L.mi_g1_ntt_device(None, None, 1, 0, None) == -1
    assert out.raw == bytes(2 * gu.AFF)


def _check_recoding(exe, tmp_path):
    vals = gu.recoding_cases(random.Random(0x61))
    assert len(vals) >= 6 + 2 * 63 + 256
    got = gu.host_recode(exe, str(tmp_path), vals)
    for t, (pos, neg) in zip(vals, got):
        assert (pos, neg) == gu.naf(t), hex(t)
        nz = pos | neg
        assert pos - neg == t and not (pos & neg) and not (nz & (nz >> 1)), hex(t)


_CASES = {}


def _transform_cases(co):
    """-> [(log_n, inverse, points)], [expected]: random points with infinity among them for log_n 0..5, and P_j = P for all j"""
    if not _CASES:
        cases, want = [], []
        for log_n in range(0, 6):
            n = 1 << log_n
            pts = bytearray(co.gen_bases("g1", 400 + log_n, n))
            for j in range(n):
                if j % 5 == 2 or (log_n == 2 and j == 0):
                    pts[gu.AFF * j:gu.AFF * (j + 1)] = gu.INF
            same = gu.point(co.gen_bases("g1", 77, 1), 0) * n
            for inverse in (False, True):
                for p in (bytes(pts), same) if log_n in (1, 3, 5) else (bytes(pts),):
                    cases.append((log_n, inverse, p))
                    want.append(gu.definition(co, p, log_n, inverse))
        _CASES["c"], _CASES["w"] = cases, want
    return _CASES["c"], _CASES["w"]


def _check_transform(co, exe, tmp_path):
    cases, want = _transform_cases(co)
    got = gu.host_transform(co, exe, str(tmp_path), cases)
    for (log_n, inverse, pts), g, w in zip(cases, got, want):
        assert g == w, (log_n, inverse)
    # P_j = P for all j: [n] P (forward) or P (inverse) in row 0, infinity as all-zero bytes everywhere else
    for (log_n, inverse, pts), w in zip(cases, want):
        if log_n and pts[:gu.AFF] * (1 << log_n) == pts and pts[:gu.AFF] != gu.INF:
            assert w[gu.AFF:] == bytes(len(w) - gu.AFF) and w[:gu.AFF] != gu.INF
            if inverse:
                assert w[:gu.AFF] == pts[:gu.AFF]


def test_host_recoding(tmp_path):
    """g1fft::recode compiled with g++ against the textbook non-adjacent form in Python: 0, 1, 2, r - 1, (r +- 1) / 2, every twiddle of
    log_n <= 6 in both directions and 256 random values; the digits sum back to t, none is adjacent to another"""
    _check_recoding(gu.host_exe(), tmp_path)


def test_host_serial_transform(co, tmp_path):
    """the level plan, index map, twiddle lookup, butterfly body and point I/O of the kernel as a serial loop over the lanes, log_n 0..5 in
    both directions, against one naive MSM of the oracle per output row"""
    _check_transform(co, gu.host_exe(), tmp_path)


def test_host_program_under_sanitizers(co, tmp_path):
    """the same stand-alone program built with -fsanitize=address,undefined and run directly: an index of a level outside its vector or its
    table, or an overflowing shift, ends the program"""
    exe = gu.host_exe(sanitize=True)
    _check_recoding(exe, tmp_path)
    _check_transform(co, exe, tmp_path)


def test_cpu_baseline_matches_definition(co, tmp_path):
    """tests/host/g1_ntt_ref.c (the baseline tools/bench_g1_ntt.py times: the oracle's Jacobian arithmetic, its own index map) against the
    same expected rows, on one thread and on three"""
    cases, want = _transform_cases(co)
    exe = gu.ref_exe()
    for (log_n, inverse, pts), w in zip(cases, want):
        if log_n == 0:
            continue
        jac, secs = gu.run_ref(exe, str(tmp_path), pts, log_n, inverse, threads=1 + 2 * (log_n & 1))
        got = b"".join(co.to_affine("g1", jac[gu.JAC * k:gu.JAC * (k + 1)]) for k in range(1 << log_n))
        assert got == w and secs > 0, (log_n, inverse)


def test_g1_ntt_kernel_resources(pkg):
    """The level kernel in the shipped code objects of both builds: no spilled VGPRs or SGPRs, at most 256 registers, and — it contains calls
    (the shared multiplier) — no AGPRs, the rule of csrc/Makefile's compiler note."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr

    for test_hooks in (False, True):
        lib = pkg.lib_path(test_hooks)
        res, calls = kr.resources(lib), kr.kernels_with_calls(lib)
        mine = {k: v for k, v in res.items() if "g1fft::" in k}
        assert sorted(k.split("(")[0] for k in mine) == ["g1fft::k_g1_ntt_level"], sorted(mine)
        for k, v in mine.items():
            assert v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (k, v)
            assert v["vgpr_count"] + v.get("agpr_count", 0) <= 256, (k, v)
            assert calls[k] and v.get("agpr_count", 0) == 0, (k, v)
            assert v["max_flat_workgroup_size"] == 64, (k, v)
