"""CPU tests of the batched inversion and the running products / sums over the scalar field (mi_fr_batch_inverse, mi_fr_scan and their device
forms): the C ABI surface, the level plan, index maps and per-lane steps of csrc/scan_kernels.cuh compiled as plain C++ and run as a serial loop
over the lanes (also under AddressSanitizer + UBSan, as a stand-alone program), the independent C++ reference the GPU tests use for large sizes,
and the resources of the kernels in the shipped code objects.  Every comparison is bit for bit against Python integers (tests/scan_util.py)."""
import ctypes as C
import os
import random
import re
import struct
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import scan_util as su  # noqa: E402

SYMS = ("mi_fr_batch_inverse", "mi_fr_batch_inverse_device", "mi_fr_scan", "mi_fr_scan_device")
R = su.R
DEFAULT_TILE_BITS = 10


def test_symbols_declared_exported_and_bound(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "arkblst_amd.h")).read(), flags=re.S)
    for s in SYMS:
        assert re.search(r"\bint\s+%s\s*\(" % s, text), s
    for test_hooks in (False, True):
        exported = subprocess.check_output(["nm", "-D", "--defined-only", pkg.lib_path(test_hooks)]).decode()
        for s in SYMS:
            assert re.search(r" T %s$" % s, exported, flags=re.M), (s, test_hooks)
    # the switch of the test build leaves no trace in the product
    assert b"MI_TEST_" not in open(pkg.lib_path(False), "rb").read()
    assert b"MI_TEST_SCAN_TILE_BITS" in open(pkg.lib_path(True), "rb").read()
    L = pkg.load_library()
    vp, sz, u, i = C.c_void_p, C.c_size_t, C.c_uint, C.c_int
    assert L.mi_fr_batch_inverse.argtypes == [vp, vp, vp, sz, u, vp, C.POINTER(sz)]
    assert L.mi_fr_batch_inverse_device.argtypes == [vp, vp, vp, sz, u, vp, C.POINTER(sz)]
    assert L.mi_fr_scan.argtypes == [vp, i, vp, sz, sz, i, u, vp, vp]
    assert L.mi_fr_scan_device.argtypes == [vp, i, vp, sz, sz, i, u, vp, vp]
    for name in ("fr_batch_inverse", "fr_batch_inverse_device", "fr_scan", "fr_scan_device"):
        assert callable(getattr(pkg.Context, name))
    for name in ("batch_inversion", "batch_inversion_and_mul", "grand_product"):
        assert callable(getattr(pkg, name)) and callable(getattr(pkg.msm, name))
    # no context: MI_E_INVALID, before anything is touched
    o, t, nz = C.create_string_buffer(b"\x5a" * 64), C.create_string_buffer(b"\x5a" * 32), C.c_size_t(77)
    assert L.mi_fr_batch_inverse(None, bytes(64), bytes(64), 2, 1, o, C.byref(nz)) == -1
    assert L.mi_fr_batch_inverse_device(None, None, None, 2, 1, None, C.byref(nz)) == -1
    assert L.mi_fr_scan(None, 0, bytes(64), 2, 1, 0, 1, o, t) == -1
    assert L.mi_fr_scan_device(None, 0, None, 2, 1, 0, 1, None, t) == -1
    assert o.raw == b"\x5a" * 64 + b"\0" and t.raw == b"\x5a" * 32 + b"\0" and nz.value == 77


# ---- the host model against Python
SCAN_MODES = (0b111, 0b110, 0b010, 0b100, 0b011)   # bit 0 in place, bit 1 out wanted, bit 2 totals wanted
INV_MODES = (0, 1, 8, 9, 24)                       # bit 0 in place over a, bit 3 numerators given, bit 4 in place over the numerators


def _sizes(tile_bits, cap=1 << 13):
    T = 1 << tile_bits
    first = [0, 1, 2, 3, T - 1, T, T + 1, 2 * T + 1, T * T - 1]
    return sorted(set(first + [n for n in (T * T, T * T + 1, T ** 3 + 1) if n <= cap]))


def _cases(tile_bits_list, big=True):
    """(kind, tile_bits, n, batch, fmt, op, exclusive, mode, variant).  Every size in both formats: the scan with both ops, inclusive and exclusive,
    the inversion three times; the batch shapes, the modes and the input variants rotate, so that each meets every level count.  Then the inputs
    that belong to one operation, at 2T + 1 elements."""
    cases, k, ki = [], 0, 0
    for tb in tile_bits_list:
        T = 1 << tb
        for n in _sizes(tb):
            if n > 1 << 13:   # 2^20 - 1 at the production tile: once each (Montgomery form, in place)
                if big:
                    cases.append(("scan", tb, n, 1, 1, su.MUL, 1, 0b111, "ones"))
                    cases.append(("inverse", tb, n, 1, 1, 0, 0, 9, "zeros"))
                continue
            for fmt in (0, 1):
                for op in (su.MUL, su.ADD):
                    for ex in (0, 1):
                        cases.append(("scan", tb, n, (1, 3)[k % 2], fmt, op, ex, SCAN_MODES[k % 5], su.VARIANTS[k % 7]))
                        k += 1
                for _ in range(3):
                    cases.append(("inverse", tb, n, 1, fmt, 0, 0, INV_MODES[ki % 5], su.VARIANTS[ki % 7]))
                    ki += 1
        n = 2 * T + 1
        for fmt in (0, 1):
            for ex in (0, 1):
                cases.append(("scan", tb, n, 3, fmt, su.MUL, ex, 0b111, "single_zero"))
                cases.append(("scan", tb, n, 1, fmt, su.ADD, ex, 0b110, "minus_one"))
            for variant in ("zeros", "zero_tile", "all_zero"):
                for mode in INV_MODES:
                    cases.append(("inverse", tb, n, 1, fmt, 0, 0, mode, variant))
    return cases


def _inputs(i, case):
    kind, tb, n, batch, fmt, op, ex, mode, variant = case
    rnd = random.Random(1000 * i + n)
    words = su.make_vector(variant, batch * n, tb, fmt, rnd)
    num = su.unpack_raw(rnd.randbytes(32 * n)) if kind == "inverse" and mode & 8 else None
    return words, num


def _run_scan_host(exe, tmp_path, cases):
    fin, fout = str(tmp_path / "scan_in.bin"), str(tmp_path / "scan_out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for i, case in enumerate(cases):
            kind, tb, n, batch, fmt, op, ex, mode, variant = case
            words, num = _inputs(i, case)
            f.write(struct.pack("<8I", int(kind == "inverse"), tb, n, batch, fmt, op, ex, mode))
            f.write(su.pack_raw(words))
            if num is not None:
                f.write(su.pack_raw(num))
    subprocess.check_call([exe, fin, fout])
    raw = open(fout, "rb").read()
    pos, levels = 0, {}
    for i, case in enumerate(cases):
        kind, tb, n, batch, fmt, op, ex, mode, variant = case
        words, num = _inputs(i, case)
        lv, got_tb = struct.unpack_from("<2I", raw, pos)
        pos += 8
        assert got_tb == tb and lv == su.levels(n, tb), case
        levels.setdefault((kind, tb), set()).add(lv)
        vals = su.values_of_raw(words, fmt)
        if kind == "inverse":
            want, want_zeros = su.batch_inverse(vals, None if num is None else su.values_of_raw(num, fmt))
            assert struct.unpack_from("<Q", raw, pos)[0] == want_zeros, case
            pos += 8
            assert raw[pos:pos + 32 * n] == su.expected_bytes(want, fmt), case
            pos += 32 * n
            continue
        want_out, want_tot = [], []
        for b in range(batch):
            o, t = su.scan(vals[b * n:(b + 1) * n], op, bool(ex))
            want_out += o
            want_tot.append(t)
        if mode & 2:
            assert raw[pos:pos + 32 * batch * n] == su.expected_bytes(want_out, fmt), ("out",) + case
            pos += 32 * batch * n
        if mode & 4:
            assert raw[pos:pos + 32 * batch] == su.expected_bytes(want_tot, fmt), ("totals",) + case
            pos += 32 * batch
    assert pos == len(raw)
    return levels


def test_host_plan_and_lane_steps(tmp_path):
    """scan_kernels.cuh compiled with g++ and run as a serial loop over workgroups and lanes: tiles of 4, 8, 16 and 1024 elements; n in 0, 1, 2, 3,
    T - 1, T, T + 1, 2T + 1, T^2 - 1, and T^2, T^2 + 1, T^3 + 1 where they stay at or below 2^13, 2^20 - 1 once at the production tile; both
    formats; the scan with both ops, inclusive and exclusive, batch 1 and 3, with and without out and totals, in place and out of place; the
    inversion with and without numerators, in place over a and over the numerators; zeros at the edges of lanes, waves and tiles, a tile and a
    vector of zeros, a single zero in a product, 1 and r - 1, r - 1 under ADD, and unreduced words"""
    cases = _cases((2, 3, 4, DEFAULT_TILE_BITS))
    scans = [c for c in cases if c[0] == "scan"]
    invs = [c for c in cases if c[0] == "inverse"]
    assert {c[7] for c in scans} == set(SCAN_MODES) and {c[3] for c in scans} == {1, 3} and {c[7] for c in invs} == set(INV_MODES)
    assert {c[8] for c in scans} == set(su.VARIANTS) == {c[8] for c in invs}
    for tb in (2, 3, 4):   # every batch shape, mode and variant of the scan, every mode of the inversion meets one, two, three and four levels
        for sel in (3, 7, 8):
            for val in {c[sel] for c in scans}:
                assert {su.levels(c[2], tb) for c in scans if c[1] == tb and c[sel] == val} >= {1, 2, 3, 4}, (tb, sel, val)
        for val in INV_MODES:
            assert {su.levels(c[2], tb) for c in invs if c[1] == tb and c[7] == val} >= {1, 2, 3, 4}, (tb, val)
    levels = _run_scan_host(su.host_exe("fr_scan_host"), tmp_path, cases)
    for kind in ("scan", "inverse"):
        for tb in (2, 3, 4):   # the reduced tile is not vacuous: one, two, three and at least four levels all occur under it
            assert {1, 2, 3} <= levels[kind, tb] and max(levels[kind, tb]) >= 4, (kind, tb, levels[kind, tb])
        assert levels[kind, DEFAULT_TILE_BITS] == {1, 2}


def test_host_program_under_sanitizers(tmp_path):
    """the same program built stand-alone with -fsanitize=address,undefined (nothing under a sanitizer is loaded into Python): every vector has
    the size the library allocates, so an index of a sweep outside its tile, level or scratch, or an overflowing shift, ends the program"""
    _run_scan_host(su.host_exe("fr_scan_host", sanitize=True), tmp_path, _cases((2, 3, 4, DEFAULT_TILE_BITS), big=False))


def test_cpp_reference_matches_python(tmp_path):
    """tests/host/fr_scan_ref.cpp (unsigned __int128 Montgomery, independent of fr.cuh) against scan_util for n <= 2^10, on one and on three
    threads"""
    exe = su.host_exe("fr_scan_ref")
    rnd = random.Random(5)
    k = 0
    for n in (0, 1, 2, 3, 31, 1 << 10):
        for fmt in (0, 1):
            for variant in ("random", "zeros", "all_zero", "single_zero", "minus_one"):
                k += 1
                threads = (1, 3)[k % 2]
                batch = (1, 3)[(k // 2) % 2]
                words = su.make_vector(variant, batch * n, 4, fmt, rnd)
                vals = su.values_of_raw(words, fmt)
                for op in (su.MUL, su.ADD):
                    for ex in (False, True):
                        res = [su.scan(vals[b * n:(b + 1) * n], op, ex) for b in range(batch)]
                        want_o = su.expected_bytes([x for o, _ in res for x in o], fmt)
                        want_t = su.expected_bytes([t for _, t in res], fmt)
                        got = su.run_ref(exe, str(tmp_path), "scan", su.pack_raw(words), n, batch, fmt, threads, op, ex)
                        assert got[:2] == (want_o, want_t), (n, fmt, variant, op, ex)
                    got = su.run_ref(exe, str(tmp_path), "scan", su.pack_raw(words), n, batch, fmt, threads, op, False, no_out=True)
                    assert got[:2] == (b"", want_t), (n, fmt, variant, op)
                a, num = words[:n], su.unpack_raw(rnd.randbytes(32 * n))
                for nm in (None, num):
                    want, zeros = su.batch_inverse(vals[:n], None if nm is None else su.values_of_raw(nm, fmt))
                    got = su.run_ref(exe, str(tmp_path), "inverse", su.pack_raw(a), n, 1, fmt, threads, num=None if nm is None else su.pack_raw(nm))
                    assert got[:2] == (su.expected_bytes(want, fmt), zeros), (n, fmt, variant, nm is not None)


def test_scan_kernels_resources(pkg):
    """The kernels of the scan namespace in the shipped code objects of both builds: the exact list, no spilled VGPRs or SGPRs, no scratch at
    all, no call in the body (the multiplier and the inversion's exponentiation are inlined) and no AGPRs, workgroups of 256 lanes, at most
    32 KiB of LDS (8 KiB for the up sweep's reduction: 256 x 32 B; 16 KiB for the scan: two copies; 32 KiB for the inversion: prefix and suffix), at most 128 VGPRs (four waves per
    SIMD; the one-workgroup kernel of the inversion's top level: 256).  The one-element-per-lane forms of the reduced tiles exist in the test build only."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr

    for test_hooks in (False, True):
        lib = pkg.lib_path(test_hooks)
        res, calls = kr.resources(lib), kr.kernels_with_calls(lib)
        mine = {k: v for k, v in res.items() if "scan::k_" in k}
        names = sorted(re.sub(r"^void ", "", k).split("(")[0] for k in mine)
        want = []
        for lanes in ("4u",) + (("1u",) if test_hooks else ()):
            want += ["scan::k_scan_up<0, %s>" % lanes, "scan::k_scan_up<1, %s>" % lanes, "scan::k_scan_down<0, %s>" % lanes,
                     "scan::k_scan_down<1, %s>" % lanes, "scan::k_inv_down<%s, false>" % lanes, "scan::k_inv_down<%s, true>" % lanes]
        assert names == sorted(want), names
        for k, v in mine.items():
            assert v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (k, v)
            assert v.get("private_segment_fixed_size", 0) == 0, (k, v)
            # the top level's inversion kernel runs ONE workgroup per call (the level one tile holds), with the four 256-bit values of the
            # binary inversion beside the lane's elements, prefix and suffix: occupancy means nothing there, and it is held to 256
            assert not calls[k] and v.get("agpr_count", 0) == 0 and v["vgpr_count"] <= (256 if "k_inv_down" in k and "true" in k else 128), (k, v)
            assert v["max_flat_workgroup_size"] == 256, (k, v)
            assert v["group_segment_fixed_size"] == (32 << 10 if "k_inv_down" in k else 16 << 10 if "k_scan_down" in k else 8 << 10), (k, v)
