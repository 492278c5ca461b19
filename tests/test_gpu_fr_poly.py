"""GPU tests of opening polynomials over the scalar field (mi_fr_poly_open, mi_fr_poly_open_device): every output is compared bit for bit —
against Python integers (tests/poly_util.py) around every boundary of a lane, a wave and a tile, against an independent C++ Horner
(tests/host/fr_poly_ref.cpp) at two levels of the production tile, against the closed form of a sparse polynomial at 2^26, and, for the
opening proof end to end, against the known-discrete-log oracle."""
import ctypes as C
import json
import os
import random
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import poly_util as pu  # noqa: E402

pytestmark = pytest.mark.gpu
R = pu.R
LANE_ELEMS = 4   # consecutive elements of one lane (csrc/poly_kernels.cuh; the C ABI does not expose it)
B_MODES = ((1, 1), (3, 1), (3, 3))   # (batch, n_points)
_REF = {}   # (n, point kind, batch, n_points) -> (coefficients, points, quotients, values) as residues, shared by both formats
_TILE = []


def _dev(data: bytes):
    import torch

    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return t


def _tile(ctx):
    """T = 2^window_bits of the product build, read from the profile"""
    if not _TILE:
        ctx.fr_poly_open(bytes(64), 2, 1, bytes(32), 1)
        p = ctx.profile()
        assert p["n"] == 2 and p["num_windows"] == 1 and 6 <= p["window_bits"] <= 12
        _TILE.append(1 << p["window_bits"])
    return _TILE[0]


def _ref(n, zk, batch, n_points):
    key = (n, zk, batch, n_points)
    if key not in _REF:
        rnd = random.Random(f"{n} {zk} {batch} {n_points}")
        coeffs = [rnd.randrange(R) for _ in range(batch * n)]
        first = {"zero": 0, "one": 1, "minus_one": R - 1}.get(zk)
        zs = [rnd.randrange(2, R) if first is None else first] + [rnd.randrange(2, R) for _ in range(n_points - 1)]
        opened = [pu.open(coeffs[b * n:(b + 1) * n], zs[b if n_points > 1 else 0]) for b in range(batch)]
        _REF[key] = (coeffs, zs, [x for q, _ in opened for x in q], [v for _, v in opened])
    return _REF[key]


def _first_diff(got, want):
    bad = [i for i in range(len(want) // 32) if got[32 * i:32 * i + 32] != want[32 * i:32 * i + 32]]
    return f"{len(bad)} of {len(want) // 32} elements differ, first at {bad[:8]}"


def _all_forms(ctx, data, n, batch, points, fmt, want_q, want_v, tag):
    """host form, device form out of place (the input stays) and in place"""
    q, v = ctx.fr_poly_open(data, n, batch, points, fmt)
    assert q == want_q and v == want_v, ("host", tag, _first_diff(q, want_q), v == want_v)
    p = ctx.profile()
    T = _tile(ctx)
    assert p["num_windows"] == (1 if n <= T else 2) and p["n"] == batch * n and 1 << p["window_bits"] == T and p["ingest_ms"] == 0, (tag, p)
    if n == 0:
        return
    d_in, d_out = _dev(data), _dev(bytes([0x5A]) * len(data))
    v = ctx.fr_poly_open_device(d_in.data_ptr(), n, batch, points, fmt, d_out.data_ptr())
    got = d_out.cpu().numpy().tobytes()
    assert got == want_q and v == want_v and d_in.cpu().numpy().tobytes() == data, ("device", tag, _first_diff(got, want_q), v == want_v)
    v = ctx.fr_poly_open_device(d_in.data_ptr(), n, batch, points, fmt, d_in.data_ptr())
    got = d_in.cpu().numpy().tobytes()
    assert got == want_q and v == want_v, ("in place", tag, _first_diff(got, want_q), v == want_v)


@pytest.mark.parametrize("fmt", [0, 1])
def test_dense_sizes_against_python(ctx, fmt):
    """sizes around one lane's elements, one wave's, one tile's and two and three tiles; the points 0, 1, r - 1 and a random one; batch 1 and 3
    with one point and with a point per polynomial; host form, device form out of place and in place; a polynomial of r - 1 and one of words that
    are not reduced; quotients NULL and values NULL; the profile reports one level up to n = T and two from T + 1"""
    T, k = _tile(ctx), LANE_ELEMS
    sizes = sorted({0, 1, 2, 3, k - 1, k, k + 1, 64 * k - 1, 64 * k + 1, T - 1, T, T + 1, 2 * T + 1, 3 * T - 1})
    for n in sizes:
        for zk in ("zero", "one", "minus_one", "random"):
            for batch, n_points in B_MODES:
                coeffs, zs, want_q, want_v = _ref(n, zk, batch, n_points)
                _all_forms(ctx, pu.pack(coeffs, fmt), n, batch, pu.pack(zs, fmt), fmt, pu.expected_bytes(want_q, fmt), pu.expected_bytes(want_v, fmt),
                           (n, zk, batch, n_points, fmt))
    rnd = random.Random(0xD0 + fmt)
    z = rnd.randrange(2, R)
    for n in (T - 1, 2 * T + 1):
        # every coefficient r - 1; then words that are not below r: r, r + 1, 2 r + 1, 2^256 - 1, 2^255 stand for their residues, the point too
        for words, zw in (([pu.raw_of_value(R - 1, fmt)] * n, pu.raw_of_value(z, fmt)),
                          ([(R, R + 1, 2 * R + 1, (1 << 256) - 1, 1 << 255)[i % 5] for i in range(n)], 2 * R + 3)):
            q, v = pu.open([pu.value_of_raw(w, fmt) for w in words], pu.value_of_raw(zw, fmt))
            _all_forms(ctx, pu.pack_raw(words), n, 1, pu.pack_raw([zw]), fmt, pu.expected_bytes(q, fmt), pu.expected_bytes([v], fmt), ("words", n, fmt))
    # one output only
    n, (batch, n_points) = 2 * T + 1, B_MODES[2]
    coeffs, zs, want_q, want_v = _ref(n, "random", batch, n_points)
    data, points = pu.pack(coeffs, fmt), pu.pack(zs, fmt)
    want_q, want_v = pu.expected_bytes(want_q, fmt), pu.expected_bytes(want_v, fmt)
    assert ctx.fr_poly_open(data, n, batch, points, fmt, quotients=False) == (None, want_v)
    assert ctx.fr_poly_open(data, n, batch, points, fmt, values=False) == (want_q, None)
    fill = bytes([0x5A]) * len(data)
    d_in, d_out = _dev(data), _dev(fill)
    assert ctx.fr_poly_open_device(d_in.data_ptr(), n, batch, points, fmt, None) == want_v
    assert d_out.cpu().numpy().tobytes() == fill and d_in.cpu().numpy().tobytes() == data
    vals = C.create_string_buffer(bytes([0x5A]) * (32 * batch), 32 * batch)
    assert ctx.fr_poly_open_device(d_in.data_ptr(), n, batch, points, fmt, d_out.data_ptr(), values=False) is None
    assert d_out.cpu().numpy().tobytes() == want_q and d_in.cpu().numpy().tobytes() == data and vals.raw == bytes([0x5A]) * (32 * batch)


@pytest.fixture(scope="module")
def ref_exe():
    return pu.host_exe("fr_poly_ref")


def test_two_levels_production_tile(ctx, ref_exe, tmp_path):
    """T^2 + 1 coefficients, the first size whose tile totals no longer fit one tile (2^22 + 1 should T^2 pass 2^24): random words, Montgomery
    form, device form, in place, against the C++ reference"""
    import numpy as np

    T = _tile(ctx)
    n = T * T + 1 if T * T <= 1 << 24 else (1 << 22) + 1
    data = np.random.default_rng(n).integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32).tobytes()
    point = pu.pack([random.Random(n).randrange(2, R)], 1)
    want_q, want_v, secs = pu.run_ref(ref_exe, str(tmp_path), data, n, 1, point, 1)
    print(f"fr_poly_ref {n}: {secs:.2f} s")
    d = _dev(data)
    v = ctx.fr_poly_open_device(d.data_ptr(), n, 1, point, 1, d.data_ptr())
    assert ctx.profile()["num_windows"] == (3 if n > T * T else 2)
    got = d.cpu().numpy().tobytes()
    assert got == want_q and v == want_v, (_first_diff(got, want_q), v == want_v)


_CHILD = r"""
import json, os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(here)r)
import poly_util as pu
import __graft_entry__ as g
pkg = g.load_package()
import random
out = {}
for tb in (2, 3, 4):
    os.environ["MI_TEST_POLY_TILE_BITS"] = str(tb)
    T = 1 << tb
    with pkg.Context([0], test_hooks=True) as c:
        for n in sorted({0, 1, 2, 3, T - 1, T, T + 1, 2 * T + 1, T * T - 1, T * T, T * T + 1, T ** 3 + 1, 4097}):
            rnd = random.Random(n)
            ok, levels = True, set()
            for k, (batch, n_points) in enumerate(((1, 1), (3, 1), (3, 3))):
                fmt = (k + n) & 1
                coeffs = [rnd.randrange(pu.R) for _ in range(batch * n)]
                zs = [rnd.randrange(pu.R) for _ in range(n_points)]
                opened = [pu.open(coeffs[b * n:(b + 1) * n], zs[b if n_points > 1 else 0]) for b in range(batch)]
                want_q = pu.expected_bytes([x for q, _ in opened for x in q], fmt)
                want_v = pu.expected_bytes([v for _, v in opened], fmt)
                data, points = pu.pack(coeffs, fmt), pu.pack(zs, fmt)
                ok = ok and c.fr_poly_open(data, n, batch, points, fmt) == (want_q, want_v)
                p = c.profile()
                ok = ok and p["window_bits"] == tb and p["n"] == batch * n
                levels.add(p["num_windows"])
                ok = ok and c.fr_poly_open(data, n, batch, points, fmt, quotients=False) == (None, want_v)
                levels.add(c.profile()["num_windows"])
            out["%%d,%%d" %% (tb, n)] = [ok, sorted(levels)]
print("RESULT " + json.dumps(out))
"""


def test_multi_level_structure_test_build():
    """test build with MI_TEST_POLY_TILE_BITS = 2, 3, 4 (contexts created in a child process, so the environment is read): n from 0 to 16^3 + 1
    around every power of the tile, batch 1 and 3, one point and a point per polynomial, opening and evaluation alone, full comparison with
    Python; the profile shows one, two, three and at least four levels under every setting"""
    r = subprocess.run([sys.executable, "-c", _CHILD % {"root": ROOT, "here": HERE}], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    res = json.loads(line[7:])
    for tb in (2, 3, 4):
        seen = set()
        mine = {int(key.split(",")[1]): val for key, val in res.items() if key.startswith(f"{tb},")}
        assert len(mine) >= 12 and 4097 in mine
        for n, (ok, levels) in mine.items():
            assert ok, (tb, n)
            assert levels == [pu.levels(n, tb)], (tb, n, levels)
            seen |= set(levels)
        assert {1, 2, 3} <= seen and max(seen) >= 4, (tb, seen)


def test_largest_size_sparse(ctx):
    """2^26 coefficients, built and checked on the device: zero except five entries, a random point, in place; rows 0, 1, T - 1, T, n / 2,
    n / 2 + 1, n - 2, n - 1 (which is zero) and 4096 random rows of the quotient against the closed form, the value against its own.  The size at
    which a byte offset no longer fits 31 bits.  Canonical integers."""
    import torch

    n, fmt = 1 << 26, 0
    T = _tile(ctx)
    rnd = random.Random(0x26)
    z = rnd.randrange(2, R)
    entries = {j: rnd.randrange(1, R) for j in (0, 1, n // 2 + 1, n - 1, rnd.randrange(2, n - 1))}
    d = torch.zeros((n, 8), dtype=torch.int32, device="cuda")
    for j, v in entries.items():
        d[j] = torch.frombuffer(bytearray(pu.pack([v], fmt)), dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    value = ctx.fr_poly_open_device(d.data_ptr(), n, 1, pu.pack([z], fmt), fmt, d.data_ptr())
    p = ctx.profile()
    assert p["n"] == n and 1 << p["window_bits"] == T and p["num_windows"] == pu.levels(n, p["window_bits"]) and (T > 1 << 12 or p["num_windows"] >= 3)
    rows = [0, 1, T - 1, T, n // 2, n // 2 + 1, n - 2, n - 1] + [rnd.randrange(n) for _ in range(4096)]
    got = d[torch.tensor(rows, device="cuda")].cpu().numpy().tobytes()
    want = pu.expected_bytes(pu.sparse_rows(entries, n, z, rows), fmt)
    assert got == want, _first_diff(got, want)
    assert got[32 * 7:32 * 8] == bytes(32)
    assert value == pu.expected_bytes([pu.sparse_value(entries, z)], fmt)


def test_kzg_opening_end_to_end(pkg, co):
    """n = 2^10: the SRS tau^i G from batch_mul_device becomes the resident base set, C = msm_device(p), (proof, v) = kzg10_open at a random z —
    with no scalar and no base on the host in between.  v = p(z), C = p(tau) G and proof = ((p(tau) - v) / (tau - z)) G by the known discrete
    logarithms."""
    n = 1 << 10
    rnd = random.Random(0x4B5A)
    tau, z = rnd.randrange(2, R), rnd.randrange(2, R)
    coeffs = [rnd.randrange(R) for _ in range(n)]
    with pkg.Context([0]) as c:
        d_tau = _dev(pu.pack([pow(tau, i, R) for i in range(n)], 1))
        d_srs = _dev(bytes(96 * n))
        c.batch_mul_device("g1", co.mul_gen("g1", 1), d_tau.data_ptr(), n, pkg.SCALAR_MONTGOMERY, d_srs.data_ptr())
        c.set_bases_device("g1", d_srs.data_ptr(), n)
        d = _dev(pu.pack(coeffs, 1))
        commitment = c.msm_device("g1", d.data_ptr(), n, pkg.SCALAR_MONTGOMERY)
        proof, value = pkg.DensePolynomial.kzg10_open(c, d.data_ptr(), n, z)
    v, p_tau = pu.evaluate(coeffs, z), pu.evaluate(coeffs, tau)
    assert value == pu.expected_bytes([v], 1)
    assert co.to_affine("g1", commitment) == co.mul_gen("g1", p_tau)
    assert co.to_affine("g1", proof) == co.mul_gen("g1", (p_tau - v) * pow(tau - z, -1, R) % R)


def test_python_and_cpp_mirrors(pkg, tmp_path):
    """DensePolynomial of msm.py on host coefficients: evaluate and divide_by_linear, integer and byte points, Montgomery by default; and of
    host/ark_blst_amd.hpp (built with g++ against the C-ABI library, run as a child process) on the same polynomial"""
    rnd = random.Random(14)
    coeffs = [rnd.randrange(R) for _ in range(37)]
    z = rnd.randrange(R)
    q, v = pu.open(coeffs, z)
    P = pkg.DensePolynomial(pu.pack(coeffs, 1))
    assert P.evaluate(z) == pu.expected_bytes([v], 1) == P.evaluate(pu.pack([z], 1))
    quotient, value = P.divide_by_linear(z)
    assert quotient.coeffs == pu.expected_bytes(q[:-1], 1) and len(quotient) == 36 and value == pu.expected_bytes([v], 1)
    P0 = pkg.DensePolynomial(pu.pack(coeffs, 0), scalar_fmt=pkg.SCALAR_CANONICAL)
    assert P0.evaluate(z) == pu.expected_bytes([v], 0) and P0.divide_by_linear(z)[0].coeffs == pu.expected_bytes(q[:-1], 0)
    for name, content in (("coeffs", pu.pack(coeffs, 1)), ("point", pu.pack([z], 1)), ("quotient", pu.expected_bytes(q[:-1], 1)), ("value", pu.expected_bytes([v], 1))):
        (tmp_path / f"{name}.bin").write_bytes(content)
    exe = os.path.join(HERE, "host", "poly_open_test")
    lib = os.path.join(ROOT, "ark-blst_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "host", "poly_open_test.cpp"), "-L" + lib, "-larkblst_amd",
                           "-Wl,-rpath," + lib])
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "DensePolynomial OK" in out.stdout, out.stdout + out.stderr


def test_arguments(pkg):
    """every MI_E_INVALID case through the raw handle: refused on the host before any launch, with every buffer untouched"""
    rnd = random.Random(9)
    n, batch = 16, 3
    data = pu.pack([rnd.randrange(R) for _ in range(batch * n)], 1)
    pts = pu.pack([rnd.randrange(R) for _ in range(batch)], 1)
    fill = bytes([0x5A])
    with pkg.Context([0]) as c, pkg.Context([0, 0]) as c2:
        L, h = c._L, c._h
        q, v = C.create_string_buffer(fill * len(data), len(data)), C.create_string_buffer(fill * (32 * batch), 32 * batch)
        bad_host = [
            (None, n, batch, pts, batch, 1, q, v), (data, n, batch, None, batch, 1, q, v),      # NULL coefficients, NULL points
            (data, n, batch, pts, batch, 1, None, None),                                            # both outputs NULL
            (data, n, batch, pts, batch, 2, q, v), (data, n, 0, pts, 1, 1, q, v),                  # scalar_fmt, batch
            (data, n, batch, pts, 2, 1, q, v), (data, n, batch, pts, 0, 1, q, v), (data, n, 1, pts, 3, 1, q, v),   # n_points
            (data, (1 << 26) + 1, 1, pts, 1, 1, q, v), (data, n, 1 << 60, pts, 1, 1, q, v), (data, 1 << 26, 1 << 40, pts, 1, 1, q, v)]
        for a in bad_host:
            assert L.mi_fr_poly_open(h, *a) == -1, a[1:6]
        assert q.raw == fill * len(data) and v.raw == fill * (32 * batch)
        d_in, d_out = _dev(data), _dev(fill * len(data))
        p_in, p_out = d_in.data_ptr(), d_out.data_ptr()
        bad_dev = [
            (0, n, batch, pts, batch, 1, p_out, v), (p_in, n, batch, None, batch, 1, p_out, v), (p_in, n, batch, pts, batch, 1, 0, None),
            (p_in, n, batch, pts, batch, 3, p_out, v), (p_in, n, 0, pts, 1, 1, p_out, v), (p_in, n, batch, pts, 2, 1, p_out, v),
            (p_in, (1 << 26) + 1, 1, pts, 1, 1, p_out, v), (p_in, n, 1 << 60, pts, 1, 1, p_out, v),
            (4096, n, batch, pts, batch, 1, p_out, v), (p_in, n, batch, pts, batch, 1, 4096, v),    # pointers the runtime does not know
            (p_in + 8, n, 1, pts, 1, 1, p_out, v), (p_in, n, 1, pts, 1, 1, p_out + 8, v),           # not 16-byte aligned
            (p_in, n, 1, pts, 1, 1, p_in + 32, v), (p_in + 32, n, 1, pts, 1, 1, p_in, v)]           # an overlap that is not identity
        for a in bad_dev:
            assert L.mi_fr_poly_open_device(h, C.c_void_p(a[0]), *a[1:6], C.c_void_p(a[6]), a[7]) == -1, a[:3] + a[4:7]
        host_ptr = C.cast(q, C.c_void_p)   # host memory where device memory is expected
        assert L.mi_fr_poly_open_device(h, host_ptr, n, batch, pts, batch, 1, C.c_void_p(p_out), v) == -1
        assert L.mi_fr_poly_open_device(h, C.c_void_p(p_in), n, batch, pts, batch, 1, host_ptr, v) == -1
        # a context of several devices has no device form
        assert c2._L.mi_fr_poly_open_device(c2._h, C.c_void_p(p_in), n, batch, pts, batch, 1, C.c_void_p(p_out), v) == -1
        assert d_in.cpu().numpy().tobytes() == data and d_out.cpu().numpy().tobytes() == fill * len(data)
        assert q.raw == fill * len(data) and v.raw == fill * (32 * batch)
        # n == 0: success, the values are zero and the quotients stay as they are
        assert L.mi_fr_poly_open(h, data, 0, batch, pts, batch, 1, q, v) == 0 and v.raw == bytes(32 * batch) and q.raw == fill * len(data)
        assert L.mi_fr_poly_open_device(h, C.c_void_p(p_in), 0, batch, pts, 1, 1, C.c_void_p(p_out), v) == 0
        assert d_out.cpu().numpy().tobytes() == fill * len(data)
        # n == 1: the one quotient slot is zero, the value is the reduced coefficient
        one = pu.pack_raw([R + 7])
        assert c.fr_poly_open(one, 1, 1, pts[:32], 1) == (bytes(32), pu.pack_raw([7]))
        # the multi-device context still opens in the host form, on its first device
        want = pu.open([pu.value_of_raw(w, 1) for w in pu.unpack_raw(data[:32 * n])], pu.value_of_raw(pu.unpack_raw(pts)[0], 1))
        assert c2.fr_poly_open(data[:32 * n], n, 1, pts[:32], 1) == (pu.expected_bytes(want[0], 1), pu.expected_bytes([want[1]], 1))
