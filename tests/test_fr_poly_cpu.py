"""CPU tests of opening polynomials over the scalar field (mi_fr_poly_open, mi_fr_poly_open_device): the C ABI surface, the level plan, index maps
and per-lane steps of csrc/poly_kernels.cuh compiled as plain C++ and run as a serial loop over the lanes (also under AddressSanitizer + UBSan, as
a stand-alone program), the independent C++ reference the GPU tests use for large sizes, and the resources of the kernels in the shipped code
objects.  Every comparison is bit for bit against Python integers (tests/poly_util.py)."""
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
import poly_util as pu  # noqa: E402

SYMS = ("mi_fr_poly_open", "mi_fr_poly_open_device")
R = pu.R
DEFAULT_TILE_BITS = 10
MINV = pow(pu.nu.MONT, -1, R)


def test_symbols_declared_exported_and_bound(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "arkblst_amd.h")).read(), flags=re.S)
    for s in SYMS:
        assert re.search(r"\bint\s+%s\s*\(" % s, text), s
    for test_hooks in (False, True):
        exported = subprocess.check_output(["nm", "-D", "--defined-only", pkg.lib_path(test_hooks)]).decode()
        for s in SYMS:
            assert re.search(r" T %s$" % s, exported, flags=re.M), (s, test_hooks)
    L = pkg.load_library()
    vp, sz, u = C.c_void_p, C.c_size_t, C.c_uint
    assert L.mi_fr_poly_open.argtypes == [vp, vp, sz, sz, vp, sz, u, vp, vp]
    assert L.mi_fr_poly_open_device.argtypes == [vp, vp, sz, sz, vp, sz, u, vp, vp]
    for name in ("fr_poly_open", "fr_poly_open_device"):
        assert callable(getattr(pkg.Context, name))
    # no context: MI_E_INVALID, before anything is touched
    q, v = C.create_string_buffer(64), C.create_string_buffer(32)
    assert L.mi_fr_poly_open(None, bytes(64), 2, 1, bytes(32), 1, 1, q, v) == -1
    assert L.mi_fr_poly_open_device(None, None, 2, 1, bytes(32), 1, 1, None, v) == -1
    assert q.raw == bytes(64) and v.raw == bytes(32)
    # the mirror of ark_poly's DensePolynomial: the refusals that need no device
    P = pkg.DensePolynomial
    assert len(P(bytes(96))) == 3 and P.MAX_COEFFS == 1 << 26
    with pytest.raises(pkg.msm.MsmErr):
        P(bytes(33))
    with pytest.raises(pkg.msm.MsmErr):
        P(bytes(64)).evaluate(bytes(31))
    with pytest.raises(pkg.msm.MsmErr):
        P(bytes(64)).divide_by_linear(bytes(64))
    with pytest.raises(pkg.msm.MsmErr):
        P.kzg10_open(None, 0, 0, 5)
    with pytest.raises(pkg.msm.MsmErr):
        P.kzg10_open(None, 0, 4, bytes(33))
    assert P(b"").evaluate(7) == bytes(32) and len(P(b"").divide_by_linear(7)[0]) == 0   # the zero polynomial never reaches the library


# ---- the host model against Python
Z_KINDS = ("zero", "one", "minus_one", "random", "non_reduced")
B_MODES = ((1, 1), (3, 1), (3, 3))                     # (batch, n_points)
P_MODES = (0b111, 0b110, 0b010, 0b100)                 # in place / out of place with both outputs, quotients only, values only


def _sizes(tile_bits, cap=1 << 13):
    T = 1 << tile_bits
    first = [0, 1, 2, 3, T - 1, T, T + 1, 2 * T + 1, T * T - 1]
    return sorted(set(first + [n for n in (T * T, T * T + 1, T ** 3 + 1) if n <= cap]))


def _z_word(kind, fmt, rnd):
    """the stored 256-bit word of a point"""
    if kind == "non_reduced":
        return rnd.choice((R + 5, 2 * R + 1, (1 << 256) - 1))
    v = {"zero": 0, "one": 1, "minus_one": R - 1}.get(kind)
    return pu.raw_of_value(rnd.randrange(2, R) if v is None else v, fmt)


def _cases(tile_bits_list, big=True):
    """every size with every kind of point in both formats; the batch shapes and the output modes rotate, so that each meets every size"""
    rnd = random.Random(0x9017)
    cases, k = [], 0
    for tb in tile_bits_list:
        for n in _sizes(tb):
            if n > 1 << 13:   # 2^20 - 1 at the production tile: once (a random point, Montgomery form, in place, both outputs)
                if big:
                    cases.append((tb, n, 1, 1, 1, 0b111, [_z_word("random", 1, rnd)]))
                continue
            for zk in Z_KINDS:
                for fmt in (0, 1):
                    batch, n_points = B_MODES[k % 3]
                    mode = P_MODES[(k // 3) % 4]
                    k += 1
                    cases.append((tb, n, batch, n_points, fmt, mode, [_z_word(zk, fmt, rnd)] + [_z_word("random", fmt, rnd) for _ in range(n_points - 1)]))
    return cases


def _words(n, seed):
    """n random 256-bit words (more than half of them not below r: every coefficient goes through the load, which reduces)"""
    return pu.unpack_raw(random.Random(seed).randbytes(32 * n))


def _run_poly_host(exe, tmp_path, cases):
    fin, fout = str(tmp_path / "poly_in.bin"), str(tmp_path / "poly_out.bin")
    data = {}
    with open(fin, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for i, (tb, n, batch, n_points, fmt, mode, zs) in enumerate(cases):
            data[i] = _words(batch * n, 31 * n + batch)
            if n >= 2:
                data[i][n - 1] = pu.raw_of_value(R - 1, fmt)
            f.write(struct.pack("<6I", tb, n, batch, n_points, fmt, mode))
            f.write(pu.pack_raw(zs))
            f.write(pu.pack_raw(data[i]))
    subprocess.check_call([exe, fin, fout])
    raw = open(fout, "rb").read()
    pos, levels = 0, {}
    for i, (tb, n, batch, n_points, fmt, mode, zs) in enumerate(cases):
        lv, got_tb = struct.unpack_from("<2I", raw, pos)
        pos += 8
        assert got_tb == tb and lv == pu.levels(n, tb), (tb, n, lv)
        levels.setdefault(tb, set()).add(lv)
        vals = [w % R * MINV % R for w in data[i]] if fmt else [w % R for w in data[i]]   # value_of_raw, its inverse taken once
        want_q, want_v = [], []
        for b in range(batch):
            q, v = pu.open(vals[b * n:(b + 1) * n], pu.value_of_raw(zs[b if n_points > 1 else 0], fmt))
            want_q += q
            want_v.append(v)
        if mode & 2:
            got = raw[pos:pos + 32 * batch * n]
            pos += 32 * batch * n
            assert got == pu.expected_bytes(want_q, fmt), ("quotients", tb, n, batch, n_points, fmt, mode)
        if mode & 4:
            got = raw[pos:pos + 32 * batch]
            pos += 32 * batch
            assert got == pu.expected_bytes(want_v, fmt), ("values", tb, n, batch, n_points, fmt, mode)
    assert pos == len(raw)
    return levels


def test_host_plan_and_lane_steps(tmp_path):
    """poly_kernels.cuh compiled with g++ and run as a serial loop over workgroups and lanes: tiles of 4, 8, 16 and 1024 elements; n in 0, 1, 2, 3,
    T - 1, T, T + 1, 2T + 1, T^2 - 1, and T^2, T^2 + 1, T^3 + 1 where they stay at or below 2^13; the points 0, 1, r - 1, a random one and a word
    that is not reduced, in both formats; batch 1 and 3 with one point and with a point per polynomial; in place and out of place, quotients only
    and values only"""
    cases = _cases((2, 3, 4, DEFAULT_TILE_BITS))
    assert {c[5] for c in cases} == set(P_MODES) and {(c[2], c[3]) for c in cases} == set(B_MODES)
    for tb in (2, 3, 4):   # every batch shape and every output mode meets sizes of one, two, three and four levels
        for sel in (2, 5):
            for val in {c[sel] for c in cases}:
                assert {pu.levels(c[1], tb) for c in cases if c[0] == tb and c[sel] == val} >= {1, 2, 3, 4}, (tb, sel, val)
    levels = _run_poly_host(pu.host_exe("fr_poly_host"), tmp_path, cases)
    for tb in (2, 3, 4):   # the reduced tile is not vacuous: one, two, three and at least four levels all occur under it
        assert {1, 2, 3} <= levels[tb] and max(levels[tb]) >= 4, (tb, levels[tb])
    assert levels[DEFAULT_TILE_BITS] == {1, 2}


def test_host_program_under_sanitizers(tmp_path):
    """the same program built stand-alone with -fsanitize=address,undefined (nothing under a sanitizer is loaded into Python): every vector has
    the size the library allocates, so an index of a sweep outside its tile, level, table or scratch, or an overflowing shift, ends the program"""
    _run_poly_host(pu.host_exe("fr_poly_host", sanitize=True), tmp_path, _cases((2, 3, 4, DEFAULT_TILE_BITS), big=False))


def test_cpp_reference_matches_python(tmp_path):
    """tests/host/fr_poly_ref.cpp (unsigned __int128 Montgomery, independent of fr.cuh) against poly_util for n <= 2^10"""
    exe = pu.host_exe("fr_poly_ref")
    rnd = random.Random(5)
    for n in (0, 1, 2, 3, 31, 1 << 10):
        for fmt in (0, 1):
            for batch, n_points in B_MODES:
                words = _words(batch * n, n + fmt)
                zs = [_z_word(Z_KINDS[(n + k) % 5], fmt, rnd) for k in range(n_points)]
                vals = [pu.value_of_raw(w, fmt) for w in words]
                opened = [pu.open(vals[b * n:(b + 1) * n], pu.value_of_raw(zs[b if n_points > 1 else 0], fmt)) for b in range(batch)]
                want_q = pu.expected_bytes([x for q, _ in opened for x in q], fmt)
                want_v = pu.expected_bytes([v for _, v in opened], fmt)
                got_q, got_v, _ = pu.run_ref(exe, str(tmp_path), pu.pack_raw(words), n, batch, pu.pack_raw(zs), fmt, threads=2)
                assert (got_q, got_v) == (want_q, want_v), (n, fmt, batch, n_points)
                got_q, got_v, _ = pu.run_ref(exe, str(tmp_path), pu.pack_raw(words), n, batch, pu.pack_raw(zs), fmt, evaluate_only=True)
                assert (got_q, got_v) == (b"", want_v), (n, fmt, batch, n_points)


def test_poly_kernels_resources(pkg):
    """The sweep kernels in the shipped code objects of both builds: no spilled VGPRs or SGPRs, no scratch at all, no call in the body (the
    multiplier is inlined) and no AGPRs, 16 KiB of LDS per workgroup of 256 lanes (two copies of the scan's 256 x 32 B), at most 128 VGPRs
    (four waves per SIMD).  The one-element-per-lane form of the reduced tiles exists in the test build only."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr

    for test_hooks in (False, True):
        lib = pkg.lib_path(test_hooks)
        res, calls = kr.resources(lib), kr.kernels_with_calls(lib)
        mine = {k: v for k, v in res.items() if "poly::k_" in k}
        names = sorted(re.sub(r"^void ", "", k).split("(")[0] for k in mine)
        want = ["poly::k_poly_down<4u>", "poly::k_poly_up<4u>"] + (["poly::k_poly_down<1u>", "poly::k_poly_up<1u>"] if test_hooks else [])
        assert names == sorted(want), names
        for k, v in mine.items():
            assert v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (k, v)
            assert v.get("private_segment_fixed_size", 0) == 0, (k, v)
            assert not calls[k] and v.get("agpr_count", 0) == 0 and v["vgpr_count"] <= 128, (k, v)
            assert v["max_flat_workgroup_size"] == 256 and v["group_segment_fixed_size"] == 16 << 10, (k, v)
