"""CPU tests of the NTT over the scalar field (mi_fr_ntt, mi_fr_ntt_device, mi_fr_vec_op_device): the C ABI surface and the constants, the Fr
arithmetic of csrc/fr.cuh and the pass structure of csrc/ntt_kernels.cuh compiled as plain C++ (also under AddressSanitizer + UBSan, as
stand-alone programs), the independent C++ reference the GPU tests use for large sizes, and the resources of the kernels in the shipped code
objects.  Every comparison is bit for bit against Python integers (tests/ntt_util.py)."""
import ctypes as C
import os
import random
import re
import struct
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import ntt_util as nu  # noqa: E402

SYMS = ("mi_fr_ntt", "mi_fr_ntt_device", "mi_fr_vec_op_device")
R = nu.R


def test_symbols_declared_exported_and_bound(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "arkblst_amd.h")).read(), flags=re.S)
    for s in SYMS:
        assert re.search(r"\bint\s+%s\s*\(" % s, text), s
    assert re.search(r"MI_FR_MUL\s*=\s*0,\s*MI_FR_ADD\s*=\s*1,\s*MI_FR_SUB\s*=\s*2", text)
    for test_hooks in (False, True):
        exported = subprocess.check_output(["nm", "-D", "--defined-only", pkg.lib_path(test_hooks)]).decode()
        for s in SYMS:
            assert re.search(r" T %s$" % s, exported, flags=re.M), (s, test_hooks)
    L = pkg.load_library()
    vp, sz, u, i = C.c_void_p, C.c_size_t, C.c_uint, C.c_int
    assert L.mi_fr_ntt.argtypes == [vp, vp, u, sz, i, vp, u, vp]
    assert L.mi_fr_ntt_device.argtypes == [vp, vp, u, sz, i, vp, u, vp]
    assert L.mi_fr_vec_op_device.argtypes == [vp, i, vp, vp, sz, u, vp]
    for name in ("fr_ntt", "fr_ntt_device", "fr_vec_op_device"):
        assert callable(getattr(pkg.Context, name))
    assert (pkg.FR_MUL, pkg.FR_ADD, pkg.FR_SUB) == (0, 1, 2)
    # no context: MI_E_INVALID, for every entry point, before anything is touched
    out = C.create_string_buffer(64)
    assert L.mi_fr_ntt(None, bytes(64), 1, 1, 0, None, 1, out) == -1
    assert L.mi_fr_ntt_device(None, None, 1, 1, 0, None, 1, None) == -1
    assert L.mi_fr_vec_op_device(None, 0, None, None, 1, 1, None) == -1
    assert out.raw == bytes(64)
    # the mirror of ark_poly's domain: sizes, and the refusals that need no device
    D = pkg.Radix2EvaluationDomain
    assert [D.new(k).size for k in (0, 1, 2, 3, 5, 1024, 1025)] == [1, 1, 2, 4, 8, 1024, 2048]
    assert D.new(1 << 26).log_size_of_group == 26 and D.new((1 << 26) + 1) is None and D.GENERATOR == 7
    with pytest.raises(pkg.msm.MsmErr):
        D.new(4).fft(bytes(32 * 5))
    with pytest.raises(pkg.msm.MsmErr):
        D.new(4).coset_ifft(bytes(31))


def test_constants_recomputed():
    """csrc/fr_consts.h (and FR_MOD / FR_INV32 of fp28_consts.h) from oracle.bls12_381.R_ORDER and the number 7 alone"""
    words = lambda v: [(v >> (32 * k)) & 0xFFFFFFFF for k in range(8)]
    got = {}
    for header in ("fr_consts.h", "fp28_consts.h"):
        text = open(os.path.join(ROOT, "ark-blst_amd", "csrc", header)).read()
        for m in re.finditer(r"static constexpr uint32_t (\w+)\[8\] = \{([^}]*)\};", text):
            got[m.group(1)] = [int(x.strip().rstrip("u"), 16) for x in m.group(2).split(",")]
        for m in re.finditer(r"static constexpr (?:uint32_t|int) (\w+) = (0x[0-9a-f]+|\d+)u?;", text):
            got[m.group(1)] = int(m.group(2), 0)
    root = pow(7, (R - 1) >> 32, R)
    assert root == 0x16A2A19EDFE81F20D09B681922C813B4B63683508C2280B93829971F439F0D2B == nu.ROOT
    assert (R - 1) % (1 << 32) == 0 and ((R - 1) >> 32) % 2 == 1 and got["TWO_ADICITY"] == 32
    mont = lambda v: words(v * (1 << 256) % R)
    assert got["FR_MOD"] == words(R) and got["FR_INV32"] == (-pow(R, -1, 1 << 32)) % (1 << 32)
    assert got["ONE"] == words((1 << 256) % R) and got["R2"] == words((1 << 512) % R)
    assert got["ROOT"] == mont(root) and got["ROOT_INV"] == mont(pow(root, -1, R))
    assert got["GEN"] == mont(7) and got["GEN_INV"] == mont(pow(7, -1, R))


def _element_pairs():
    rnd = random.Random(0xF7)
    edge = nu.edge_operands()
    pairs = [(a, b) for a in edge for b in edge]
    pairs += [(a, b) for a in nu.load_only_operands() for b in (0, 1, R - 1)]
    pairs += [(rnd.randrange(R), rnd.randrange(R)) for _ in range(200)]
    return pairs


def _run_fr_host_check(exe, tmp_path):
    pairs = _element_pairs()
    fin, fout = str(tmp_path / "fr_in.bin"), str(tmp_path / "fr_out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<Q", len(pairs)))
        for a, b in pairs:
            f.write(nu.pack_raw([a, b]))
    subprocess.check_call([exe, fin, fout])
    got = nu.unpack_raw(open(fout, "rb").read())
    assert len(got) == 10 * len(pairs)
    assert all(x < R for x in got)
    minv = pow(nu.MONT, -1, R)
    for k, (a, b) in enumerate(pairs):
        want = []
        for fmt in (0, 1):
            x, y = nu.value_of_raw(a, fmt), nu.value_of_raw(b, fmt)
            want += [nu.raw_of_value(x * y, fmt), nu.raw_of_value(x + y, fmt), nu.raw_of_value(x - y, fmt)]
        want += [a % R * nu.MONT % R, a % R * minv % R, a % R * nu.MONT % R, a % R]
        assert got[10 * k:10 * k + 10] == want, (k, hex(a), hex(b))


def test_host_fr_arithmetic(tmp_path):
    """fr.cuh compiled with g++: mul / add / sub / to and from Montgomery / both load formats on every pair of the edge operands, the
    non-reduced loads and 200 random pairs; every result below r.  Before that the program checks fr::load_scalar (the scalar prologue of
    the MSM digit kernels) on its own: nine edge inputs, both formats, fold on and off, against 64-bit limb arithmetic restated in it"""
    _run_fr_host_check(nu.host_exe("fr_host_check"), tmp_path)


_MODES = [(False, None), (True, None), (False, 7), (True, 7), (False, "rnd"), (True, "rnd")]
_VALS, _WANT = {}, {}   # the reference transforms, computed once per (log_n, direction, offset) and packed once per format


def _case(log_n, inverse, offset, fmt, batch=3):
    """-> (input bytes, expected bytes, offset bytes or None) of `batch` random vectors"""
    key = (log_n, inverse, offset)
    if key not in _VALS:
        rnd = random.Random(1000 * log_n + 10 * int(inverse) + len(str(offset)))
        g = rnd.randrange(1, R) if offset == "rnd" else offset
        vals = [[rnd.randrange(R) for _ in range(1 << log_n)] for _ in range(batch)]
        vals[-1][0] = R - 1
        _VALS[key] = (vals, [nu.transform(v, inverse, g) for v in vals], g)
    if key + (fmt,) not in _WANT:
        vals, outs, g = _VALS[key]
        _WANT[key + (fmt,)] = (b"".join(nu.pack(v, fmt) for v in vals), b"".join(nu.expected_bytes(v, fmt) for v in outs),
                               None if g is None else nu.pack([g], fmt))
    return _WANT[key + (fmt,)]


def _run_ntt_host(exe, tmp_path, log_ns, caps, in_place_too=True):
    cases = []
    for log_n in log_ns:
        for cap in caps:
            for inverse, offset in _MODES:
                fmt = (log_n + cap + int(inverse)) & 1
                for in_place in ((0, 1) if in_place_too else (0,)):
                    cases.append((log_n, cap, inverse, offset, fmt, in_place))
    fin, fout = str(tmp_path / "ntt_in.bin"), str(tmp_path / "ntt_out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for log_n, cap, inverse, offset, fmt, in_place in cases:
            data, _, g = _case(log_n, inverse, offset, fmt)
            f.write(struct.pack("<7I", log_n, cap, 3, int(inverse), int(g is not None), fmt, in_place))
            f.write(g if g is not None else bytes(32))
            f.write(data)
    subprocess.check_call([exe, fin, fout])
    raw = open(fout, "rb").read()
    pos, passes = 0, {}
    for log_n, cap, inverse, offset, fmt, in_place in cases:
        _, want, _ = _case(log_n, inverse, offset, fmt)
        p, widest = struct.unpack_from("<2I", raw, pos)
        got = raw[pos + 8:pos + 8 + len(want)]
        pos += 8 + len(want)
        assert got == want, (log_n, cap, inverse, offset, fmt, in_place)
        assert widest <= min(cap, 7) and p >= -(-log_n // min(cap, 7)) and (not in_place or p < 3 or p % 2 == 0)
        passes[(log_n, cap, in_place)] = p
    assert pos == len(raw)
    return passes


def test_host_pass_plan_and_index_maps(tmp_path):
    """ntt_kernels.cuh compiled with g++ and run as a serial loop over workgroups and lanes: every log_n 0..12 with the levels per pass capped
    at 1, 2, 3 and uncapped; forward, inverse, coset with offset 7 and a random offset; batch 3; out of place and in place; both formats"""
    passes = _run_ntt_host(nu.host_exe("fr_ntt_host"), tmp_path, range(0, 13), (1, 2, 3, 7))
    assert passes[(12, 7, 0)] == 2 and passes[(7, 7, 0)] == 1 and passes[(8, 7, 0)] == 2 and passes[(0, 7, 0)] == 1
    for cap in (1, 2, 3):   # the cap is not vacuous: one, two, three and at least four passes all occur under it
        seen = {p for (log_n, c, ip), p in passes.items() if c == cap}
        assert {1, 2, 3} <= seen and max(seen) >= 4, (cap, seen)
    assert passes[(12, 3, 0)] == 4 and passes[(9, 3, 0)] == 3 and passes[(9, 3, 1)] == 4   # in place: an even number of passes from three on


def test_host_programs_under_sanitizers(tmp_path):
    """the same two programs built stand-alone with -fsanitize=address,undefined (nothing under a sanitizer is loaded into Python): an index
    of a pass outside its tile, vector or table, or an overflowing shift, ends the program"""
    _run_fr_host_check(nu.host_exe("fr_host_check", sanitize=True), tmp_path)
    _run_ntt_host(nu.host_exe("fr_ntt_host", sanitize=True), tmp_path, (0, 1, 2, 3, 4, 7, 8, 10, 11), (1, 3, 7))


def test_cpp_reference_matches_python(tmp_path):
    """tests/host/fr_ntt_ref.cpp (unsigned __int128 Montgomery, independent of fr.cuh) against ntt_util for log_n <= 10"""
    exe = nu.host_exe("fr_ntt_ref")
    for log_n in (0, 1, 2, 5, 10):
        for inverse, offset in _MODES:
            fmt = (log_n + int(inverse)) & 1
            data, want, g = _case(log_n, inverse, offset, fmt)
            got, _ = nu.run_ref(exe, str(tmp_path), data, log_n, 3, inverse, g, fmt, threads=2)
            assert got == want, (log_n, inverse, offset, fmt)


def test_ntt_kernels_resources(pkg):
    """The NTT kernels in the shipped code objects of both builds: no spilled VGPRs or SGPRs, no scratch at all (so none inside the butterfly
    loops), no call in the body (the multiplier is inlined) and no AGPRs, 32 KiB of LDS per workgroup of 256 lanes."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr

    for test_hooks in (False, True):
        lib = pkg.lib_path(test_hooks)
        res, calls = kr.resources(lib), kr.kernels_with_calls(lib)
        mine = {k: v for k, v in res.items() if "ntt::k_" in k}
        assert sorted(k.split("(")[0] for k in mine) == ["ntt::k_fr_powers", "ntt::k_fr_vec_op", "ntt::k_ntt_pass"], sorted(mine)
        for k, v in mine.items():
            assert v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (k, v)
            assert v.get("private_segment_fixed_size", 0) == 0, (k, v)
            assert not (calls[k] and v.get("agpr_count", 0) > 0) and v["vgpr_count"] + v.get("agpr_count", 0) <= 256, (k, v)
            assert v["max_flat_workgroup_size"] == 256, (k, v)
        pass_k = [v for k, v in mine.items() if "k_ntt_pass" in k][0]
        assert pass_k["group_segment_fixed_size"] == 32 << 10 and pass_k["vgpr_count"] <= 128, pass_k   # at least four waves per SIMD
    hot = kr.HOT
    try:
        kr.HOT = ("ntt::k_ntt_pass",)
        loops = kr.scratch_in_hot_loops(pkg.lib_path())
    finally:
        kr.HOT = hot
    assert len(loops) == 1 and not any(loops.values()), loops
