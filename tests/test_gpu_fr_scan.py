"""GPU tests of the batched inversion and the running products / sums over the scalar field (mi_fr_batch_inverse, mi_fr_scan and their device
forms): every output is compared bit for bit — against Python integers (tests/scan_util.py) around every boundary of a lane, a wave and a tile,
against an independent C++ loop (tests/host/fr_scan_ref.cpp) at two levels of the production tile, against closed forms of an almost constant
vector at 2^26, and, for the grand product of a permutation argument end to end, against the known-discrete-log oracle."""
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
import scan_util as su  # noqa: E402

pytestmark = pytest.mark.gpu
R = su.R
MUL, ADD = su.MUL, su.ADD
LANE_ELEMS = 4   # consecutive elements of one lane (csrc/scan_kernels.cuh; the C ABI does not expose it)
_TILE = []
FILL = bytes([0x5A])


def _dev(data: bytes):
    import torch

    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return t


def _host(t) -> bytes:
    return t.cpu().numpy().tobytes()


def _tile(ctx):
    """T = 2^window_bits of the product build, read from the profile"""
    if not _TILE:
        ctx.fr_scan(MUL, bytes(64), 2)
        p = ctx.profile()
        assert p["n"] == 2 and p["num_windows"] == 1 and 6 <= p["window_bits"] <= 12
        _TILE.append(1 << p["window_bits"])
    return _TILE[0]


def _first_diff(got, want):
    bad = [i for i in range(len(want) // 32) if got[32 * i:32 * i + 32] != want[32 * i:32 * i + 32]]
    return f"{len(bad)} of {len(want) // 32} elements differ, first at {bad[:8]}"


def _profile_ok(ctx, n, total, tag):
    p = ctx.profile()
    T = _tile(ctx)
    assert p["num_windows"] == su.levels(n, p["window_bits"]) == (1 if n <= T else 2) and p["n"] == total and 1 << p["window_bits"] == T, (tag, p)
    assert p["ingest_ms"] == 0, (tag, p)


def _scan_all_forms(ctx, op, words, n, batch, ex, fmt, tag):
    """host form, device form out of place (the input stays) and in place, and the reduction alone"""
    data = su.pack_raw(words)
    vals = su.values_of_raw(words, fmt)
    res = [su.scan(vals[b * n:(b + 1) * n], op, ex) for b in range(batch)]
    want_o, want_t = su.expected_bytes([x for o, _ in res for x in o], fmt), su.expected_bytes([t for _, t in res], fmt)
    o, t = ctx.fr_scan(op, data, n, batch, ex, fmt)
    assert o == want_o and t == want_t, ("host", tag, _first_diff(o, want_o), t == want_t)
    _profile_ok(ctx, n, batch * n, tag)
    assert ctx.fr_scan(op, data, n, batch, ex, fmt, out=False) == (None, want_t), ("host, totals only", tag)
    if n == 0:
        return
    d_in, d_out = _dev(data), _dev(FILL * len(data))
    t = ctx.fr_scan_device(op, d_in.data_ptr(), n, batch, ex, fmt, d_out.data_ptr())
    got = _host(d_out)
    assert got == want_o and t == want_t and _host(d_in) == data, ("device", tag, _first_diff(got, want_o), t == want_t)
    _profile_ok(ctx, n, batch * n, tag)
    assert ctx.fr_scan_device(op, d_in.data_ptr(), n, batch, ex, fmt, None) == want_t and _host(d_in) == data, ("device, totals only", tag)
    assert ctx.fr_scan_device(op, d_in.data_ptr(), n, batch, ex, fmt, d_in.data_ptr(), totals=False) is None
    got = _host(d_in)
    assert got == want_o, ("in place", tag, _first_diff(got, want_o))


def _inverse_all_forms(ctx, words, num, fmt, tag):
    """host form, device form out of place (the inputs stay), in place over a and over the numerators"""
    n = len(words)
    a, nm = su.pack_raw(words), None if num is None else su.pack_raw(num)
    want, zeros = su.batch_inverse(su.values_of_raw(words, fmt), None if num is None else su.values_of_raw(num, fmt))
    want = su.expected_bytes(want, fmt)
    o, z = ctx.fr_batch_inverse(a, nm, fmt)
    assert o == want and z == zeros, ("host", tag, _first_diff(o, want), z, zeros)
    _profile_ok(ctx, n, n, tag)
    if n == 0:
        return
    d_a, d_out = _dev(a), _dev(FILL * len(a))
    d_n = None if nm is None else _dev(nm)
    p_n = None if nm is None else d_n.data_ptr()
    z = ctx.fr_batch_inverse_device(d_a.data_ptr(), p_n, n, fmt, d_out.data_ptr())
    got = _host(d_out)
    assert got == want and z == zeros and _host(d_a) == a and (nm is None or _host(d_n) == nm), ("device", tag, _first_diff(got, want), z, zeros)
    _profile_ok(ctx, n, n, tag)
    if nm is not None:
        assert ctx.fr_batch_inverse_device(d_a.data_ptr(), p_n, n, fmt, p_n) == zeros
        got = _host(d_n)
        assert got == want and _host(d_a) == a, ("in place over num", tag, _first_diff(got, want))
        d_n = _dev(nm)
        p_n = d_n.data_ptr()
    assert ctx.fr_batch_inverse_device(d_a.data_ptr(), p_n, n, fmt, d_a.data_ptr()) == zeros
    got = _host(d_a)
    assert got == want, ("in place over a", tag, _first_diff(got, want))


@pytest.mark.parametrize("fmt", [0, 1])
def test_dense_sizes_against_python(ctx, fmt):
    """sizes around one lane's elements, one wave's, one tile's and two and three tiles; both ops, inclusive and exclusive, batch 1 and 3; the
    inversion with and without numerators; host form, device form out of place and in place, totals alone; the input variants rotate over the
    sizes, and every variant (zeros at the edges of lanes, waves and tiles, a tile and a vector of zeros, a single zero in a product, 1 and r - 1,
    r - 1 under ADD, unreduced words) runs at T - 1, 2T + 1 and 3T - 1; the zero count and the profile's level count are checked"""
    T, k = _tile(ctx), LANE_ELEMS
    tb = T.bit_length() - 1
    sizes = sorted({0, 1, 2, 3, k - 1, k, k + 1, 64 * k - 1, 64 * k + 1, T - 1, T, T + 1, 2 * T + 1, 3 * T - 1})
    rnd = random.Random(0x5CA0 + fmt)
    j = 0
    for n in sizes:
        for op in (MUL, ADD):
            for ex in (False, True):
                for batch in (1, 3):
                    variant = su.VARIANTS[j % 7]
                    j += 1
                    _scan_all_forms(ctx, op, su.make_vector(variant, batch * n, tb, fmt, rnd), n, batch, ex, fmt, (n, op, ex, batch, variant, fmt))
        for with_num in (False, True):
            variant = su.VARIANTS[j % 7]
            j += 1
            num = su.unpack_raw(rnd.randbytes(32 * n)) if with_num else None
            _inverse_all_forms(ctx, su.make_vector(variant, n, tb, fmt, rnd), num, fmt, (n, with_num, variant, fmt))
    for n in (T - 1, 2 * T + 1, 3 * T - 1):
        for variant in su.VARIANTS:
            words = su.make_vector(variant, n, tb, fmt, rnd)
            num = su.make_vector("zeros", n, tb, fmt, rnd)   # a zero numerator over a zero and over a non-zero denominator, unreduced numerators
            _inverse_all_forms(ctx, words, None, fmt, (n, False, variant, fmt))
            _inverse_all_forms(ctx, words, num, fmt, (n, True, variant, fmt))
            _scan_all_forms(ctx, MUL, words, n, 1, n % 2 == 1 and variant != "zeros", fmt, (n, MUL, variant, fmt))
            _scan_all_forms(ctx, ADD, words, n, 1, variant == "zeros", fmt, (n, ADD, variant, fmt))


@pytest.fixture(scope="module")
def ref_exe():
    return su.host_exe("fr_scan_ref")


def test_two_levels_production_tile(ctx, ref_exe, tmp_path):
    """T^2 + 1 elements, the first size whose tile totals no longer fit one tile (2^22 + 1 should T^2 pass 2^24): random words with a few zeros,
    Montgomery form, device form, against the C++ reference: the inversion with numerators in place, the exclusive product scan in place"""
    import numpy as np

    T = _tile(ctx)
    n = T * T + 1 if T * T <= 1 << 24 else (1 << 22) + 1
    levels = 3 if n > T * T else 2
    rng = np.random.default_rng(n)
    a = rng.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)
    for row in (0, 5, T - 1, T, n // 2, n - 1):
        a[row] = 0
    a, num = a.tobytes(), rng.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32).tobytes()
    want, zeros, secs = su.run_ref(ref_exe, str(tmp_path), "inverse", a, n, 1, 1, 4, num=num)
    print(f"fr_scan_ref inverse {n}: {secs:.2f} s")
    assert zeros == 6
    d_a, d_n = _dev(a), _dev(num)
    assert ctx.fr_batch_inverse_device(d_a.data_ptr(), d_n.data_ptr(), n, 1, d_a.data_ptr()) == zeros
    assert ctx.profile()["num_windows"] == levels
    got = _host(d_a)
    assert got == want and _host(d_n) == num, _first_diff(got, want)
    want, want_t, secs = su.run_ref(ref_exe, str(tmp_path), "scan", num, n, 1, 1, 4, MUL, True)
    print(f"fr_scan_ref scan {n}: {secs:.2f} s")
    total = ctx.fr_scan_device(MUL, d_n.data_ptr(), n, 1, True, 1, d_n.data_ptr())
    assert ctx.profile()["num_windows"] == levels
    got = _host(d_n)
    assert got == want and total == want_t, (_first_diff(got, want), total == want_t)


_CHILD = r"""
import json, os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(here)r)
import scan_util as su
import __graft_entry__ as g
pkg = g.load_package()
import random
out = {}
for tb in (2, 3, 4):
    os.environ["MI_TEST_SCAN_TILE_BITS"] = str(tb)
    T = 1 << tb
    with pkg.Context([0], test_hooks=True) as c:
        for n in sorted({0, 1, 2, 3, T - 1, T, T + 1, 2 * T + 1, T * T - 1, T * T, T * T + 1, T ** 3 + 1, 4097}):
            rnd = random.Random(n)
            ok, levels = True, set()
            for k in range(4):
                fmt, batch, op, ex = (k + n) & 1, (1, 3)[k & 1], (su.MUL, su.ADD)[k >> 1], bool((k + (n >> 1)) & 1)
                variant = su.VARIANTS[(n + 3 * k) %% 7]
                words = su.make_vector(variant, batch * n, tb, fmt, rnd)
                vals = su.values_of_raw(words, fmt)
                res = [su.scan(vals[b * n:(b + 1) * n], op, ex) for b in range(batch)]
                want_o = su.expected_bytes([x for o, _ in res for x in o], fmt)
                want_t = su.expected_bytes([t for _, t in res], fmt)
                ok = ok and c.fr_scan(op, su.pack_raw(words), n, batch, ex, fmt) == (want_o, want_t)
                p = c.profile()
                ok = ok and p["window_bits"] == tb and p["n"] == batch * n
                levels.add(p["num_windows"])
                ok = ok and c.fr_scan(op, su.pack_raw(words), n, batch, ex, fmt, out=False) == (None, want_t)
                levels.add(c.profile()["num_windows"])
                a = words[:n]
                num = su.unpack_raw(rnd.randbytes(32 * n)) if k & 1 else None
                want, zeros = su.batch_inverse(vals[:n], None if num is None else su.values_of_raw(num, fmt))
                got = c.fr_batch_inverse(su.pack_raw(a), None if num is None else su.pack_raw(num), fmt)
                ok = ok and got == (su.expected_bytes(want, fmt), zeros)
                p = c.profile()
                ok = ok and p["window_bits"] == tb and p["n"] == n
                levels.add(p["num_windows"])
            out["%%d,%%d" %% (tb, n)] = [ok, sorted(levels)]
print("RESULT " + json.dumps(out))
"""


def test_multi_level_structure_test_build():
    """test build with MI_TEST_SCAN_TILE_BITS = 2, 3, 4 (contexts created in a child process, so the environment is read): n from 0 to 16^3 + 1
    around every power of the tile and 4097, both ops, inclusive and exclusive, batch 1 and 3, the reduction alone, the inversion with and
    without numerators, every input variant, full comparison with Python; the profile shows one, two, three and at least four levels under every
    setting"""
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
            assert levels == [su.levels(n, tb)], (tb, n, levels)
            seen |= set(levels)
        assert {1, 2, 3} <= seen and max(seen) >= 4, (tb, seen)


def _constant_vector(n, c, specials, fmt):
    import torch

    d = torch.frombuffer(bytearray(su.pack([c], fmt)), dtype=torch.int32).cuda().repeat(n, 1)
    for j, v in specials.items():
        d[j] = torch.frombuffer(bytearray(su.pack([v], fmt)), dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    return d


def test_largest_size_almost_constant(ctx):
    """2^26 elements, built and checked on the device: every element a constant c except five entries at 0, 1, n / 2 + 1, n - 1 and a random row
    (one of them zero for the inversion); rows 0, 1, T - 1, T, n / 2, n / 2 + 1, n - 2, n - 1 and 4096 random rows against the closed forms — c^-1
    for the inversion, c^(i + 1) times the specials' ratios for the inclusive product scan — and the total against its own.  The size at which a
    byte offset no longer fits 31 bits.  Canonical integers, in place."""
    import torch

    n, fmt = 1 << 26, 0
    T = _tile(ctx)
    rnd = random.Random(0x26)
    c = rnd.randrange(2, R)
    at = (0, 1, n // 2 + 1, n - 1, rnd.randrange(2, n - 1))
    rows = [0, 1, T - 1, T, n // 2, n // 2 + 1, n - 2, n - 1, at[4]] + [rnd.randrange(n) for _ in range(4096)]
    idx = torch.tensor(rows, device="cuda")

    def check_profile():
        p = ctx.profile()
        assert p["n"] == n and 1 << p["window_bits"] == T and p["num_windows"] == su.levels(n, p["window_bits"]) and (T > 1 << 12 or p["num_windows"] >= 3)

    specials = {j: rnd.randrange(1, R) for j in at}
    specials[n // 2 + 1] = 0
    d = _constant_vector(n, c, specials, fmt)
    assert ctx.fr_batch_inverse_device(d.data_ptr(), None, n, fmt, d.data_ptr()) == 1
    check_profile()
    got = d[idx].cpu().numpy().tobytes()
    want = su.expected_bytes(su.sparse_inverse_rows(c, specials, rows), fmt)
    assert got == want, _first_diff(got, want)
    del d
    specials = {j: rnd.randrange(1, R) for j in at}
    d = _constant_vector(n, c, specials, fmt)
    total = ctx.fr_scan_device(MUL, d.data_ptr(), n, 1, False, fmt, d.data_ptr())
    check_profile()
    got = d[idx].cpu().numpy().tobytes()
    want = su.expected_bytes(su.sparse_scan_rows(c, specials, MUL, False, rows), fmt)
    assert got == want, _first_diff(got, want)
    assert total == su.expected_bytes([su.sparse_scan_total(c, specials, MUL, n)], fmt)


def test_grand_product_end_to_end(pkg, co):
    """n = 2^10, a permutation argument with no scalar on the host between its steps: a permutation made of cycles, wire values constant on each
    cycle, num = w + beta id + gamma and den = w + beta sigma + gamma uploaded; grand_product on the device gives z (Python's), the total 1 and
    no zero; z[i+1] den[i] == z[i] num[i] by mi_fr_vec_op_device; then the inverse NTT and the MSM over a batch_mul_device SRS: the commitment
    is z(tau) G by the known discrete logarithms"""
    import ntt_util as nu

    n = 1 << 10
    rnd = random.Random(0x6A0D)
    beta, gamma, tau = rnd.randrange(2, R), rnd.randrange(2, R), rnd.randrange(2, R)
    order = list(range(n))
    rnd.shuffle(order)
    ident = [rnd.randrange(R) for _ in range(n)]   # distinct labels of the positions
    sigma, w, lo = [0] * n, [0] * n, 0
    while lo < n:   # cycles of random lengths over the shuffled positions
        ln = min(n - lo, rnd.randrange(1, 40))
        cyc, val = order[lo:lo + ln], rnd.randrange(R)
        for k, i in enumerate(cyc):
            sigma[i], w[i] = ident[cyc[(k + 1) % ln]], val
        lo += ln
    num = [(w[i] + beta * ident[i] + gamma) % R for i in range(n)]
    den = [(w[i] + beta * sigma[i] + gamma) % R for i in range(n)]
    z, total = su.scan(su.batch_inverse(den, num)[0], MUL, True)
    assert total == 1 and len(set(z)) > n // 2
    with pkg.Context([0]) as c:
        d_tau = _dev(su.pack([pow(tau, i, R) for i in range(n)], 1))
        d_srs = _dev(bytes(96 * n))
        c.batch_mul_device("g1", co.mul_gen("g1", 1), d_tau.data_ptr(), n, pkg.SCALAR_MONTGOMERY, d_srs.data_ptr())
        c.set_bases_device("g1", d_srs.data_ptr(), n)
        d_num, d_den, d_z = _dev(su.pack(num, 1)), _dev(su.pack(den, 1)), _dev(FILL * (32 * n))
        got_total, zeros = pkg.grand_product(c, d_num.data_ptr(), d_den.data_ptr(), n, d_z.data_ptr())
        assert _host(d_z) == su.expected_bytes(z, 1) and got_total == su.expected_bytes([1], 1) and zeros == 0
        assert _host(d_num) == su.pack(num, 1) and _host(d_den) == su.pack(den, 1)
        d_l, d_r = _dev(bytes(32 * (n - 1))), _dev(bytes(32 * (n - 1)))
        c.fr_vec_op_device(pkg.FR_MUL, d_z.data_ptr() + 32, d_den.data_ptr(), n - 1, 1, d_l.data_ptr())
        c.fr_vec_op_device(pkg.FR_MUL, d_z.data_ptr(), d_num.data_ptr(), n - 1, 1, d_r.data_ptr())
        assert _host(d_l) == _host(d_r) != bytes(32 * (n - 1))
        c.fr_ntt_device(d_z.data_ptr(), 10, 1, True, None, 1, d_z.data_ptr())
        commitment = c.msm_device("g1", d_z.data_ptr(), n, pkg.SCALAR_MONTGOMERY)
    z_tau = 0
    for coeff in reversed(nu.ifft(z)):
        z_tau = (z_tau * tau + coeff) % R
    assert co.to_affine("g1", commitment) == co.mul_gen("g1", z_tau)


def test_python_and_cpp_mirrors(pkg, tmp_path):
    """batch_inversion, batch_inversion_and_mul and grand_product of msm.py on a 37-element vector with two zeros, both formats; and of
    host/ark_blst_amd.hpp (built with g++ against the C-ABI library, run as a child process) on the same vectors"""
    rnd = random.Random(15)
    v = [rnd.randrange(R) for _ in range(37)]
    v[3] = v[36] = 0
    coeffs = [rnd.randrange(R) for _ in range(37)]
    inv, zeros = su.batch_inverse(v)
    quot = su.batch_inverse(v, coeffs)[0]
    z, total = su.scan(quot, MUL, True)
    for fmt in (1, 0):
        kw = {} if fmt else {"scalar_fmt": pkg.SCALAR_CANONICAL}
        assert pkg.batch_inversion(su.pack(v, fmt), **kw) == su.expected_bytes(inv, fmt)
        assert pkg.batch_inversion_and_mul(su.pack(v, fmt), su.pack(coeffs, fmt), **kw) == su.expected_bytes(quot, fmt)
        assert pkg.batch_inversion_and_mul(su.pack(v, fmt), su.pack([7], fmt), **kw) == su.expected_bytes([7 * x % R for x in inv], fmt)
    assert pkg.batch_inversion(b"") == b""
    with pytest.raises(pkg.msm.MsmErr):
        pkg.batch_inversion(bytes(33))
    with pytest.raises(pkg.msm.MsmErr):
        pkg.batch_inversion_and_mul(bytes(64), bytes(96))
    with pkg.Context([0]) as c:
        d_num, d_den = _dev(su.pack(coeffs, 1)), _dev(su.pack(v, 1))
        assert pkg.grand_product(c, d_num.data_ptr(), d_den.data_ptr(), 37, d_den.data_ptr()) == (su.expected_bytes([total], 1), zeros)
        assert _host(d_den) == su.expected_bytes(z, 1)
        with pytest.raises(pkg.msm.MsmErr):
            pkg.grand_product(c, d_num.data_ptr(), d_den.data_ptr(), 0, d_den.data_ptr())
    for name, content in (("v", su.pack(v, 1)), ("coeffs", su.pack(coeffs, 1)), ("inverse", su.expected_bytes(inv, 1)), ("quotient", su.expected_bytes(quot, 1)),
                          ("z", su.expected_bytes(z, 1)), ("total", su.expected_bytes([total], 1)), ("zeros", zeros.to_bytes(8, "little"))):
        (tmp_path / f"{name}.bin").write_bytes(content)
    exe = os.path.join(HERE, "host", "scan_mirror_test")
    lib = os.path.join(ROOT, "ark-blst_amd", "lib")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-o", exe,
                           os.path.join(HERE, "host", "scan_mirror_test.cpp"), "-L" + lib, "-larkblst_amd", "-L" + os.path.join(rocm, "lib"), "-lamdhip64",
                           "-Wl,-rpath," + lib, "-Wl,-rpath," + os.path.join(rocm, "lib")])
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "batch_inversion OK" in out.stdout, out.stdout + out.stderr


def test_arguments(pkg):
    """every MI_E_INVALID case through the raw handle: refused on the host before any launch, with every buffer untouched; the n == 0 results;
    the host forms on a context of two devices"""
    rnd = random.Random(9)
    n, batch = 16, 3
    data = su.pack([rnd.randrange(1, R) for _ in range(batch * n)], 1)
    size = len(data)
    with pkg.Context([0]) as c, pkg.Context([0, 0]) as c2:
        L, h = c._L, c._h
        o, t = C.create_string_buffer(FILL * size, size), C.create_string_buffer(FILL * (32 * batch), 32 * batch)
        nz = C.c_size_t(77)
        pz = C.byref(nz)
        # ---- the scan, host form: (op, in, n, batch, exclusive, fmt, out, totals)
        bad = [(0, None, n, batch, 0, 1, o, t), (0, data, n, batch, 0, 1, None, None),                   # NULL in, both outputs NULL
               (0, data, n, batch, 0, 2, o, t), (2, data, n, batch, 0, 1, o, t), (3, data, n, batch, 0, 1, o, t), (-1, data, n, batch, 0, 1, o, t),
               (0, data, n, batch, 2, 1, o, t), (0, data, n, batch, -1, 1, o, t), (0, data, n, 0, 0, 1, o, t),   # exclusive, batch
               (0, data, (1 << 26) + 1, 1, 0, 1, o, t), (0, data, n, 1 << 60, 0, 1, o, t), (0, data, 1 << 26, 1 << 40, 0, 1, o, t)]
        for a in bad:
            assert L.mi_fr_scan(h, *a) == -1, a[:1] + a[2:6]
        # ---- the inversion, host form: (a, num, n, fmt, out, n_zero)
        bad = [(None, None, n, 1, o, pz), (data, None, n, 1, None, pz), (data, None, n, 2, o, pz), (data, data, (1 << 26) + 1, 1, o, pz)]
        for a in bad:
            assert L.mi_fr_batch_inverse(h, *a) == -1, a[2:4]
        assert o.raw == FILL * size and t.raw == FILL * (32 * batch) and nz.value == 77
        d_in, d_out = _dev(data), _dev(FILL * size)
        p_in, p_out = d_in.data_ptr(), d_out.data_ptr()
        vp = C.c_void_p
        # ---- the scan, device form
        bad = [(0, 0, n, batch, 0, 1, p_out, t), (0, p_in, n, batch, 0, 1, 0, None), (0, p_in, n, batch, 0, 3, p_out, t), (2, p_in, n, batch, 0, 1, p_out, t),
               (0, p_in, n, batch, 2, 1, p_out, t), (0, p_in, n, 0, 0, 1, p_out, t), (0, p_in, (1 << 26) + 1, 1, 0, 1, p_out, t),
               (0, p_in, n, 1 << 60, 0, 1, p_out, t),
               (0, 4096, n, batch, 0, 1, p_out, t), (0, p_in, n, batch, 0, 1, 4096, t),                  # pointers the runtime does not know
               (0, p_in + 8, n, 1, 0, 1, p_out, t), (0, p_in, n, 1, 0, 1, p_out + 8, t),                 # not 16-byte aligned
               (0, p_in, n, 1, 0, 1, p_in + 32, t), (0, p_in + 32, n, 1, 0, 1, p_in, t)]                 # an overlap that is not identity
        for a in bad:
            assert L.mi_fr_scan_device(h, a[0], vp(a[1]), *a[2:6], vp(a[6]), a[7]) == -1, a[:7]
        host_ptr = C.cast(o, vp)   # host memory where device memory is expected
        assert L.mi_fr_scan_device(h, 0, host_ptr, n, batch, 0, 1, vp(p_out), t) == -1
        assert L.mi_fr_scan_device(h, 0, vp(p_in), n, batch, 0, 1, host_ptr, t) == -1
        # ---- the inversion, device form: (d_a, d_num, n, fmt, d_out, n_zero)
        p_num = p_in + 32 * n   # the second vector of the buffer as numerators
        bad = [(0, 0, n, 1, p_out), (p_in, 0, n, 1, 0), (p_in, 0, n, 2, p_out), (p_in, p_num, (1 << 26) + 1, 1, p_out),
               (4096, 0, n, 1, p_out), (p_in, 4096, n, 1, p_out), (p_in, 0, n, 1, 4096),
               (p_in + 8, 0, n, 1, p_out), (p_in, p_num + 8, n, 1, p_out), (p_in, 0, n, 1, p_out + 8),
               (p_in, 0, n, 1, p_in + 32), (p_in + 32, 0, n, 1, p_in), (p_in, p_num, n, 1, p_num + 32), (p_in, p_num, n, 1, p_num - 32)]
        for a in bad:
            assert L.mi_fr_batch_inverse_device(h, vp(a[0]), vp(a[1]), a[2], a[3], vp(a[4]), pz) == -1, a
        assert L.mi_fr_batch_inverse_device(h, host_ptr, None, n, 1, vp(p_out), pz) == -1
        assert L.mi_fr_batch_inverse_device(h, vp(p_in), host_ptr, n, 1, vp(p_out), pz) == -1
        assert L.mi_fr_batch_inverse_device(h, vp(p_in), None, n, 1, host_ptr, pz) == -1
        # a context of several devices has no device form
        assert c2._L.mi_fr_scan_device(c2._h, 0, vp(p_in), n, batch, 0, 1, vp(p_out), t) == -1
        assert c2._L.mi_fr_batch_inverse_device(c2._h, vp(p_in), None, n, 1, vp(p_out), pz) == -1
        assert _host(d_in) == data and _host(d_out) == FILL * size
        assert o.raw == FILL * size and t.raw == FILL * (32 * batch) and nz.value == 77
        # n == 0: success; out stays as it is; the totals are the identity in scalar_fmt; no zeros
        one = {0: su.expected_bytes([1], 0), 1: su.expected_bytes([1], 1)}
        for fmt in (0, 1):
            assert L.mi_fr_scan(h, 0, None, 0, batch, 0, fmt, o, t) == 0 and t.raw == one[fmt] * batch and o.raw == FILL * size
            assert L.mi_fr_scan(h, 1, data, 0, batch, 1, fmt, o, t) == 0 and t.raw == bytes(32 * batch) and o.raw == FILL * size
            assert L.mi_fr_scan_device(h, 0, vp(p_in), 0, batch, 1, fmt, vp(p_out), t) == 0 and t.raw == one[fmt] * batch
            assert L.mi_fr_scan_device(h, 1, None, 0, 1, 0, fmt, None, t) == 0 and t.raw[:32] == bytes(32)
        assert L.mi_fr_batch_inverse(h, None, None, 0, 1, None, pz) == 0 and nz.value == 0
        nz.value = 77
        assert L.mi_fr_batch_inverse_device(h, vp(p_in), None, 0, 1, vp(p_out), pz) == 0 and nz.value == 0
        assert L.mi_fr_batch_inverse(h, data, None, 0, 1, o, None) == 0   # the count is optional
        assert _host(d_out) == FILL * size and o.raw == FILL * size
        # the multi-device context still runs the host forms, on its first device
        vals = su.values_of_raw(su.unpack_raw(data[:32 * n]), 1)
        want, total = su.scan(vals, MUL, True)
        assert c2.fr_scan(MUL, data[:32 * n], n, 1, True, 1) == (su.expected_bytes(want, 1), su.expected_bytes([total], 1))
        assert c2.fr_batch_inverse(data[:32 * n], None, 1) == (su.expected_bytes(su.batch_inverse(vals)[0], 1), 0)
        assert c.fr_batch_inverse(data[:32 * n], None, 1, into=None)[1] == 0
