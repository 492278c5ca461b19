"""GPU tests of the fixed-base batch multiplication out[i] = s_i * P (mi_g{1,2}_batch_mul, mi_g{1,2}_batch_mul_device): byte equality of
the affine output against the C oracle (generator: co.gen_bases over the seed's discrete logs) and the Python big-int oracle (every other
base, every special scalar).  No tolerance, every output of every case is compared."""
import ctypes as C
import os
import random
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import batch_mul_util as bu  # noqa: E402

pytestmark = pytest.mark.gpu

GROUPS = ["g1", "g2"]
_EXPECT = {}   # (group, base bytes, s mod r) -> affine bytes from the big-int oracle, shared by every test of the module


def _curve(o, group):
    return (o.F1, o.G1_GEN, 96) if group == "g1" else (o.F2, o.G2_GEN, 192)


def _dlogs(co, seed, n):
    buf = C.create_string_buffer(32 * max(n, 1))
    co.lib().orc_gen_dlogs(seed, n, buf)
    return buf.raw[:32 * n]


def _want(o, group, pt, vals):
    """big-int oracle: (s mod r) * pt for every s, as packed affine bytes"""
    F, _, aff = _curve(o, group)
    key_pt = o.affine_to_bytes(F, pt)
    out = []
    for s in vals:
        k = (group, key_pt, s % o.R_ORDER)
        if k not in _EXPECT:
            q = o.scalar_mul(F, pt, s % o.R_ORDER) if pt is not o.INF else o.INF
            _EXPECT[k] = o.affine_to_bytes(F, q) if q is not o.INF else bytes(aff)
        out.append(_EXPECT[k])
    return b"".join(out)


def _assert_points(got, want, aff, what):
    assert len(got) == len(want), what
    if got != want:
        bad = [i for i in range(len(want) // aff) if got[aff * i:aff * (i + 1)] != want[aff * i:aff * (i + 1)]]
        raise AssertionError(f"{what}: {len(bad)} of {len(want) // aff} points differ, first at {bad[:8]}")


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("fmt", [0, 1])
def test_generator_shapes(ctx, pkg, co, group, fmt):
    """wave, workgroup and product-tree fan-out boundaries, both scalar formats"""
    aff = 96 if group == "g1" else 192
    gen = co.mul_gen(group, 1)
    for n in (0, 1, 63, 64, 65, 257, 1500):
        seed = 0xFB00 + n
        sc = _dlogs(co, seed, n)
        got = ctx.batch_mul(group, gen, co.fr_to_mont(sc) if fmt and n else sc, fmt)
        _assert_points(got, co.gen_bases(group, seed, n, 8), aff, (group, fmt, n))


@pytest.mark.parametrize("group", GROUPS)
def test_generator_host_form_in_ragged_chunks(ctx, co, group):
    """2^17 + 3 scalars through the host form: several chunks, none a multiple of anything; a second call reuses table and staging"""
    import numpy as np

    aff = 96 if group == "g1" else 192
    n, seed = (1 << 17) + 3, 0xFB17
    sc = _dlogs(co, seed, n)
    want = co.gen_bases(group, seed, n, 8)
    _assert_points(ctx.batch_mul(group, co.mul_gen(group, 1), sc, 0), want, aff, (group, n))
    into = np.zeros(n * aff, dtype=np.uint8)
    ctx.batch_mul(group, co.mul_gen(group, 1), sc, 0, into=into)
    assert ctx.profile()["ingest_ms"] == 0.0
    _assert_points(into.tobytes(), want, aff, (group, n, "into"))


def test_generator_g1_user_size(ctx, co):
    n, seed = 1 << 20, 0xFB20
    sc = _dlogs(co, seed, n)
    got = ctx.batch_mul("g1", co.mul_gen("g1", 1), sc, 0)
    _assert_points(got, co.gen_bases("g1", seed, n, 8), 96, ("g1", n))


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("w", list(bu.W_SUPPORTED) + [0])
def test_every_window_size(pkg, co, o, group, w):
    """every table geometry the setter accepts, then the built-in choice again: 300 dlog scalars against the C oracle plus the special
    scalars of that geometry (the constructed collisions of every geometry included) against the big-int oracle"""
    F, gen_pt, aff = _curve(o, group)
    gen = co.mul_gen(group, 1)
    seed = 0xFB30 + w
    sc = _dlogs(co, seed, 300)
    vals = bu.special_scalars(w or 10, o.R_ORDER)
    with pkg.Context([0]) as c:
        if w == 0:
            c.set_batch_mul_window_bits(16)
            c.batch_mul(group, gen, sc, 0)
            assert c.profile()["window_bits"] == 16
        c.set_batch_mul_window_bits(w)
        got = c.batch_mul(group, gen, sc + bu.scalar_bytes(vals), 0)
        p = c.profile()
        if w:
            assert p["window_bits"] == w and p["num_windows"] == bu.windows(w) and p["work_items"] == bu.windows(w) << (w - 1) and p["ingest_ms"] > 0
        else:
            assert p["window_bits"] == 16 and p["ingest_ms"] == 0.0   # w = 0 keeps a larger resident table of the same base ...
            c.batch_mul(group, co.mul_gen(group, 2), sc, 0)
            assert 8 <= c.profile()["window_bits"] < 16                # ... and chooses by n for a new base
        _assert_points(got, co.gen_bases(group, seed, 300, 8) + _want(o, group, gen_pt, vals), aff, (group, w))
        for bad in (1, 7, 17, 255):
            with pytest.raises(pkg.MsmError) as e:
                c.set_batch_mul_window_bits(bad)
            assert e.value.code == -1


@pytest.mark.parametrize("group", GROUPS)
def test_special_scalars(ctx, co, o, group):
    """group-order edges, digit-sign boundaries and carry chains of every window, all digits at the half value, the constructed collisions:
    on the generator and on one random subgroup point, in both scalar formats"""
    F, gen_pt, aff = _curve(o, group)
    r = o.R_ORDER
    other = o.scalar_mul(F, gen_pt, random.Random(31).randrange(1, r))
    vals = bu.special_scalars(10, r) + bu.special_scalars(16, r)
    for s in (bu.collision_scalar(w, r) for w in (9, 12, 14)):
        assert s is not None and 0 < s < r
    for pt in (gen_pt, other):
        want = _want(o, group, pt, vals)
        base = o.affine_to_bytes(F, pt)
        _assert_points(ctx.batch_mul(group, base, bu.scalar_bytes(vals), 0), want, aff, (group, "canonical"))
        mont = co.fr_to_mont(bu.scalar_bytes([v % r for v in vals]))
        _assert_points(ctx.batch_mul(group, base, mont, 1), want, aff, (group, "montgomery"))


@pytest.mark.parametrize("group", GROUPS)
def test_bases_that_are_not_the_generator(ctx, pkg, co, o, group):
    """integer semantics for ANY curve point: infinity, points outside the subgroup, points of small order (where almost every step of
    the walk is an exceptional pair and many table entries are infinity); a point off the curve is MI_E_INVALID"""
    from cofactor_util import off_subgroup_points, small_order_points

    F, gen_pt, aff = _curve(o, group)
    r = o.R_ORDER
    rnd = random.Random(41)
    vals = [rnd.randrange(1 << 256) for _ in range(8)] + [rnd.randrange(r) for _ in range(8)] + [rnd.randrange(1 << 20) for _ in range(4)]
    vals += [0, 1, 2, 3, 10, 11, 13, 23, r - 1, r, r + 1, (r - 1) // 2, (1 << 255) - 1, (1 << 256) - 1, 1 << 10, (1 << 10) - 1, 1 << 9, (1 << 9) + 1,
             sum(512 << (10 * j) for j in range(26)) % (1 << 256)]
    vals += [s for s in (bu.collision_scalar(w, r) for w in (9, 12, 14))]
    sc = bu.scalar_bytes(vals)
    assert ctx.batch_mul(group, bytes(aff), sc, 0) == bytes(aff * len(vals))
    for pt in off_subgroup_points(o, group, 3) + small_order_points(o, group):
        got = ctx.batch_mul(group, o.affine_to_bytes(F, pt), sc, 0)
        _assert_points(got, _want(o, group, pt, vals), aff, (group, pt))
    off = bytearray(o.affine_to_bytes(F, gen_pt))
    off[48 if group == "g1" else 96] ^= 1          # another y: not on the curve
    with pytest.raises(pkg.MsmError) as e:
        ctx.batch_mul(group, bytes(off), sc, 0)
    assert e.value.code == -1
    with pytest.raises(pkg.MsmError) as e:
        ctx.batch_mul(group, o.affine_to_bytes(F, gen_pt), sc, 2)    # unknown scalar_fmt
    assert e.value.code == -1


@pytest.mark.parametrize("group", GROUPS)
def test_table_reuse(pkg, co, o, group):
    """A, A, B, -A, A: every result is right; the context keeps the table of the LAST base, keyed by its exact bytes — the second call with
    A builds nothing (mi_profile.ingest_ms, the table build of the call, is 0), every other call rebuilds"""
    F, gen_pt, aff = _curve(o, group)
    r = o.R_ORDER
    rnd = random.Random(51)
    A = o.scalar_mul(F, gen_pt, rnd.randrange(1, r))
    B = o.scalar_mul(F, gen_pt, rnd.randrange(1, r))
    vals = [rnd.randrange(r) for _ in range(30)] + [0, 1, r - 1]
    sc = bu.scalar_bytes(vals)
    with pkg.Context([0]) as c:
        built = []
        for pt in (A, A, B, o.aff_neg(F, A), A):
            got = c.batch_mul(group, o.affine_to_bytes(F, pt), sc, 0)
            _assert_points(got, _want(o, group, pt, vals), aff, group)
            built.append(c.profile()["ingest_ms"] > 0)
        assert built == [True, False, True, True, True]


@pytest.mark.parametrize("group", GROUPS)
def test_device_forms_and_the_chain(pkg, co, o, group):
    """scalars and points in device memory; the output goes straight into set_bases_device and an MSM over it equals the closed form"""
    import torch

    aff = 96 if group == "g1" else 192
    n, seed = 5000, 0xFB60
    sc = _dlogs(co, seed, n)
    gen = co.mul_gen(group, 1)
    with pkg.Context([0]) as c:
        host = c.batch_mul(group, gen, sc, 0)
        _assert_points(host, co.gen_bases(group, seed, n, 8), aff, (group, "host"))
        d_sc = torch.frombuffer(bytearray(sc), dtype=torch.uint8).cuda()
        d_out = torch.full((n * aff,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        c.batch_mul_device(group, gen, d_sc.data_ptr(), n, 0, d_out.data_ptr())
        _assert_points(d_out.cpu().numpy().tobytes(), host, aff, (group, "device"))
        c.set_bases_device(group, d_out.data_ptr(), n)
        msc = co.gen_scalars(0xFB61, n)
        got = c.msm(group, None, msc, n, 0)
        assert co.to_affine(group, got) == co.dlog_expected(group, msc, seed, n)
        d_msc = torch.frombuffer(bytearray(msc), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        assert co.to_affine(group, c.msm_device(group, d_msc.data_ptr(), n, 0)) == co.dlog_expected(group, msc, seed, n)
        # all-zero base in the device form, n == 0, and pointers that are not device memory
        c.batch_mul_device(group, bytes(aff), d_sc.data_ptr(), n, 0, d_out.data_ptr())
        assert d_out.cpu().numpy().tobytes() == bytes(n * aff)
        c.batch_mul_device(group, gen, 0, 0, 0, 0)
        for args in ((4096, d_out.data_ptr()), (d_sc.data_ptr(), 4096)):
            with pytest.raises(pkg.MsmError) as e:
                c.batch_mul_device(group, gen, args[0], n, 0, args[1])
            assert e.value.code == -1


def test_python_and_cpp_mirrors(pkg, co, o, tmp_path):
    """G{1,2}Projective.batch_mul of msm.py (Montgomery scalars by default, the MsmErr convention) and of host/ark_blst_amd.hpp (built with
    g++ against the C-ABI library, run as a child process) on 100 scalars"""
    for group in GROUPS:
        F, gen_pt, aff = _curve(o, group)
        seed = 0xFB70
        sc = _dlogs(co, seed, 100)
        want = co.gen_bases(group, seed, 100, 4)
        P = pkg.G1Projective if group == "g1" else pkg.G2Projective
        _assert_points(P.batch_mul(co.mul_gen(group, 1), co.fr_to_mont(sc)), want, aff, group)
        _assert_points(P.batch_mul(co.mul_gen(group, 1), sc, scalar_fmt=pkg.SCALAR_CANONICAL), want, aff, group)
        assert P.batch_mul(co.mul_gen(group, 1), b"") == b""
        bad = bytearray(co.mul_gen(group, 1))
        bad[0] ^= 1
        with pytest.raises(pkg.msm.MsmErr) as e:
            P.batch_mul(bytes(bad), sc)
        assert e.value.value == 0
        (tmp_path / f"{group}_base.bin").write_bytes(co.mul_gen(group, 1))
        (tmp_path / f"{group}_scalars_mont.bin").write_bytes(co.fr_to_mont(sc))
        (tmp_path / f"{group}_expected.bin").write_bytes(want)
    exe = os.path.join(HERE, "host", "batch_mul_test")
    lib = os.path.join(ROOT, "ark-blst_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "host", "batch_mul_test.cpp"), "-L" + lib, "-larkblst_amd",
                           "-Wl,-rpath," + lib])
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "g1 batch_mul OK" in out.stdout and "g2 batch_mul OK" in out.stdout
