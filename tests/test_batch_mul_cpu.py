"""CPU tests of the fixed-base batch multiplication (mi_g{1,2}_batch_mul): the C ABI surface, the window-size model, the walk's hot and
cold paths compiled as plain C++ from the device headers, and the resources of the walk kernels in the shipped code objects."""
import ctypes as C
import os
import random
import re
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import batch_mul_util as bu  # noqa: E402

SYMS = ("mi_g1_batch_mul", "mi_g2_batch_mul", "mi_g1_batch_mul_device", "mi_g2_batch_mul_device", "mi_batch_mul_set_window_bits")


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
    for g in ("g1", "g2"):
        assert getattr(L, f"mi_{g}_batch_mul").argtypes == [vp, vp, vp, sz, u, vp]
        assert getattr(L, f"mi_{g}_batch_mul_device").argtypes == [vp, vp, vp, sz, u, vp]
    assert L.mi_batch_mul_set_window_bits.argtypes == [vp, u]
    for name in ("batch_mul", "batch_mul_device", "set_batch_mul_window_bits"):
        assert callable(getattr(pkg.Context, name))
    assert callable(pkg.G1Projective.batch_mul) and callable(pkg.G2Projective.batch_mul)
    # no context: MI_E_INVALID, for every entry point, before anything is touched
    out = C.create_string_buffer(192)
    assert L.mi_g1_batch_mul(None, bytes(96), bytes(32), 1, 0, out) == -1
    assert L.mi_g2_batch_mul(None, bytes(192), bytes(32), 1, 0, out) == -1
    assert L.mi_g1_batch_mul(None, None, None, 0, 0, None) == -1
    assert L.mi_g1_batch_mul_device(None, bytes(96), None, 1, 0, None) == -1
    assert L.mi_g2_batch_mul_device(None, bytes(192), None, 1, 0, None) == -1
    assert L.mi_batch_mul_set_window_bits(None, 8) == -1
    with pytest.raises(pkg.msm.MsmErr):
        pkg.G1Projective.batch_mul(bytes(95), bytes(32))


def test_window_model_standalone():
    """fixed_base_model.hpp compiled alone with g++ (no HIP): W w covers 255 bits plus the carry, the table stays under the documented cap and
    the chosen w is monotone for EVERY n from 1 to 2^26 (tests/host/fixed_base_model.cpp); the Python restatement agrees on the geometry."""
    exe = os.path.join(HERE, "host", "fixed_base_model")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "host", "fixed_base_model.cpp")])
    out = subprocess.check_output([exe]).decode()
    assert "fixed-base model OK" in out, out
    pick = lambda n, g2: int(subprocess.check_output([exe, "choose", str(n), str(g2)]).decode())
    for g2 in (0, 1):
        ws = [pick(1 << k, g2) for k in range(0, 27)]
        assert ws == sorted(ws) and ws[0] >= 8 and ws[-1] == 16, ws           # small n: a small table; 2^26 scalars: the fewest additions
        assert bu.windows(ws[0]) << (ws[0] - 1 + (8 if g2 else 7)) <= 4 << 20   # n = 1 does not pay for more than an L2's worth of table
    for w in bu.W_SUPPORTED:
        assert bu.windows(w) * w >= 256 and (bu.windows(w) - 1) * w <= 255
        assert (bu.windows(w) << (w - 1)) * 256 <= 128 << 20


@pytest.fixture(scope="module")
def fbw():
    so = os.path.join(HERE, "host", "libfixed_base_walk.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "host", "fixed_base_walk.cpp")])
    L = C.CDLL(so)
    L.fbw_g1.argtypes = [C.c_char_p, C.c_uint, C.c_char_p, C.c_size_t, C.c_char_p, C.c_char_p]
    return L


def _order3_point(o):
    """a point of order 3 on E(Fp): y^2 = x^3 + 4 has (0, 2)"""
    pt = (0, 2)
    assert o.on_curve(o.F1, pt) and o.scalar_mul(o.F1, pt, 3) is o.INF
    return pt


def test_recoding_and_collision_scalars(o):
    r = o.R_ORDER
    rnd = random.Random(4)
    for w in bu.W_SUPPORTED:
        for s in [0, 1, r - 1, (r - 1) // 2] + [rnd.randrange(r) for _ in range(50)]:
            d = bu.recode(s, w)
            assert len(d) == bu.windows(w) and all(-(1 << (w - 1)) < x <= (1 << (w - 1)) for x in d) and d[-1] >= 0
    have = {w: bu.collision_scalar(w, r) for w in bu.W_SUPPORTED}
    assert sorted(w for w, s in have.items() if s is not None) == [9, 12, 14]
    for w, s in have.items():
        if s is None:
            continue
        d = bu.recode(s, w)
        B = 1 << (w * (bu.windows(w) - 1))
        v = sum(x << (w * j) for j, x in enumerate(d[:-1]))
        assert 0 < s < r and (v - d[-1] * B) % r == 0 and v != d[-1] * B   # running sum == top entry as points, not as integers


@pytest.mark.parametrize("w", [8, 9, 12, 14, 16])
def test_walk_hot_and_cold_paths_on_the_host(fbw, co, o, w):
    """k_fb_walk's structure over a host-built table (tests/host/fixed_base_walk.cpp: the table recurrences of the build kernels, the
    XYZZ hot loop, the complete cold path; the recoding is restated there) against the big-int oracle: the special scalars, the
    constructed collision (the cold path RUNS on a prime-order base where one exists) and a base of order 3."""
    r = o.R_ORDER
    rnd = random.Random(100 + w)
    vals = [v % r for v in bu.special_scalars(w, r)] + [rnd.randrange(r) for _ in range(20)]
    n = len(vals)
    sc = bu.scalar_bytes(vals)
    for name, pt in (("generator", o.G1_GEN), ("order 3", _order3_point(o))):
        out, cold = C.create_string_buffer(144 * n), C.create_string_buffer(n)
        assert fbw.fbw_g1(o.affine_to_bytes(o.F1, pt), w, sc, n, out, cold) == 0
        for i, s in enumerate(vals):
            want = o.scalar_mul(o.F1, pt, s)
            want_b = o.affine_to_bytes(o.F1, want) if want is not o.INF else bytes(96)
            assert co.to_affine("g1", out.raw[144 * i:144 * (i + 1)]) == want_b, (name, w, i, hex(s))
        took = {vals[i] for i in range(n) if cold.raw[i]}
        if name == "generator":
            s = bu.collision_scalar(w, r)
            assert took == ({s} if s is not None else set()), (w, [hex(x) for x in took])
        else:
            assert len(took) > n // 2          # order 3: almost every walk meets P + P or P - P


def test_walk_kernels_resources(pkg):
    """The walk kernels in the shipped code objects of both builds: no spilled VGPRs or SGPRs, a call in the body, hence at most 256
    registers and no AGPRs; and no scratch instruction inside their arithmetic loops (kernel_resources.scratch_in_hot_loops)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr

    for test_hooks in (False, True):
        lib = pkg.lib_path(test_hooks)
        res, calls = kr.resources(lib), kr.kernels_with_calls(lib)
        walk = {k: v for k, v in res.items() if "msmk::k_fb_walk" in k}
        assert len(walk) == 2 and any("k_fb_walk<msmk::G1C>" in k for k in walk) and any("k_fb_walk_g2_coop" in k for k in walk), sorted(walk)
        for k, v in walk.items():
            assert v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (k, v)
            assert calls[k] and v["vgpr_count"] <= 256 and v.get("agpr_count", 0) == 0, (k, v)
            assert v[".max_flat_workgroup_size"[1:]] == 64, (k, v)   # workgroups of one wave
    hot = kr.HOT
    try:
        kr.HOT = ("msmk::k_fb_walk",)
        loops = kr.scratch_in_hot_loops(pkg.lib_path())
    finally:
        kr.HOT = hot
    assert len(loops) == 2 and not any(loops.values()), loops
