"""GPU tests of the NTT over the scalar field (mi_fr_ntt, mi_fr_ntt_device) and of mi_fr_vec_op_device: every output is compared bit for
bit — against Python integers (tests/ntt_util.py) up to two levels beyond one pass, against an independent C++ transform
(tests/host/fr_ntt_ref.cpp) at sizes of three passes and at 2^22, and against the closed form of a sparse vector at 2^26."""
import json
import os
import random
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import ntt_util as nu  # noqa: E402

pytestmark = pytest.mark.gpu
R = nu.R
MODES = [(False, None), (True, None), (False, 7), (True, 7)]   # fft, ifft, coset_fft, coset_ifft with arkworks' default offset
_REF = {}   # (log_n, inverse, offset) -> (three input vectors, their transforms) as residues, shared by the tests of the module


def _ref(log_n, inverse, offset):
    key = (log_n, inverse, offset)
    if key not in _REF:
        rnd = random.Random(77 * log_n + 7 * int(inverse) + (offset or 0))
        vals = [[rnd.randrange(R) for _ in range(1 << log_n)] for _ in range(3)]
        vals[1] = [R - 1] * (1 << log_n)
        _REF[key] = (vals, [nu.transform(v, inverse, offset) for v in vals])
    return _REF[key]


def _offset_bytes(offset, fmt):
    return None if offset is None else nu.pack([offset], fmt)


def _dev(data: bytes):
    import torch

    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return t


_LEVELS = []


def _levels(ctx):
    """levels of one full pass, read from the profile: the widest pass over sizes of which one is a whole number of full passes"""
    if not _LEVELS:
        widest = 0
        for log_n in range(8, 17):
            ctx.fr_ntt(bytes(32 << log_n), log_n, 1, False, None, 1)
            p = ctx.profile()
            assert p["n"] == 1 << log_n and p["num_windows"] * p["window_bits"] >= log_n
            widest = max(widest, p["window_bits"])
        assert 4 <= widest <= 8
        _LEVELS.append(widest)
    return _LEVELS[0]


def _first_diff(got, want):
    bad = [i for i in range(len(want) // 32) if got[32 * i:32 * i + 32] != want[32 * i:32 * i + 32]]
    return f"{len(bad)} of {len(want) // 32} elements differ, first at {bad[:8]}"


@pytest.mark.parametrize("fmt", [0, 1])
def test_element_ops(ctx, pkg, fmt):
    """fr_mul / fr_add / fr_sub on the GPU at chosen operands: all ordered pairs of the edge operands (two of them not below r), the
    load-only operands against 0, 1, r - 1, and 200 random pairs; out of place, and with the output on either input"""
    rnd = random.Random(0xE1 + fmt)
    edge = nu.edge_operands()
    pairs = [(a, b) for a in edge for b in edge] + [(a, b) for a in nu.load_only_operands() for b in (0, 1, R - 1)]
    pairs += [(rnd.randrange(R), rnd.randrange(R)) for _ in range(200)]
    n = len(pairs)
    a_bytes, b_bytes = nu.pack_raw(p[0] for p in pairs), nu.pack_raw(p[1] for p in pairs)
    va, vb = [nu.value_of_raw(p[0], fmt) for p in pairs], [nu.value_of_raw(p[1], fmt) for p in pairs]
    for op, f in ((pkg.FR_MUL, lambda x, y: x * y), (pkg.FR_ADD, lambda x, y: x + y), (pkg.FR_SUB, lambda x, y: x - y)):
        want = nu.expected_bytes([f(x, y) for x, y in zip(va, vb)], fmt)
        for alias in ("none", "a", "b"):
            d_a, d_b = _dev(a_bytes), _dev(b_bytes)
            d_o = {"none": _dev(bytes([0xA5]) * (32 * n)), "a": d_a, "b": d_b}[alias]
            ctx.fr_vec_op_device(op, d_a.data_ptr(), d_b.data_ptr(), n, fmt, d_o.data_ptr())
            got = d_o.cpu().numpy().tobytes()
            assert got == want, (op, fmt, alias, _first_diff(got, want))


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("inverse,offset", MODES)
def test_against_python_product_build(ctx, fmt, inverse, offset):
    """every log_n from 0 to two levels beyond one pass: random vectors and a vector of r - 1, batch 1 and 3, host form, device form out of
    place and in place; plus one vector of non-reduced entries"""
    levels = _levels(ctx)
    g = _offset_bytes(offset, fmt)
    for log_n in range(0, levels + 3):
        vals, outs = _ref(log_n, inverse, offset)
        for batch in (1, 3):
            data = b"".join(nu.pack(v, fmt) for v in vals[:batch])
            want = b"".join(nu.expected_bytes(v, fmt) for v in outs[:batch])
            got = ctx.fr_ntt(data, log_n, batch, inverse, g, fmt)
            assert got == want, ("host", log_n, batch, _first_diff(got, want))
            p = ctx.profile()
            assert p["num_windows"] == max(1, -(-log_n // levels)) and p["window_bits"] <= levels and p["n"] == batch << log_n
            d_in, d_out = _dev(data), _dev(bytes([0x5A]) * len(data))
            ctx.fr_ntt_device(d_in.data_ptr(), log_n, batch, inverse, g, fmt, d_out.data_ptr())
            got = d_out.cpu().numpy().tobytes()
            assert got == want and d_in.cpu().numpy().tobytes() == data, ("device", log_n, batch, _first_diff(got, want))
            ctx.fr_ntt_device(d_in.data_ptr(), log_n, batch, inverse, g, fmt, d_in.data_ptr())
            got = d_in.cpu().numpy().tobytes()
            assert got == want, ("in place", log_n, batch, _first_diff(got, want))
        # entries that are not below r: r, r + 1, 2 r + 1, 2^256 - 1, ... stand for their residues
        words = [(R, R + 1, 2 * R, 2 * R + 1, (1 << 256) - 1, 1 << 255)[i % 6] for i in range(1 << log_n)]
        res = nu.transform([nu.value_of_raw(w, fmt) for w in words], inverse, offset)
        got = ctx.fr_ntt(nu.pack_raw(words), log_n, 1, inverse, g, fmt)
        assert got == nu.expected_bytes(res, fmt), ("non-reduced", log_n)


_CHILD = r"""
import json, os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(here)r)
import ntt_util as nu
import __graft_entry__ as g
pkg = g.load_package()
import random
out = {}
for cap in (1, 2, 3):
    os.environ["MI_TEST_NTT_TILE_BITS"] = str(cap)
    with pkg.Context([0], test_hooks=True) as c:
        for log_n in range(0, 11):
            rnd = random.Random(log_n)
            vals = [[rnd.randrange(nu.R) for _ in range(1 << log_n)] for _ in range(2)]
            ok, passes = True, set()
            for k, (inverse, offset) in enumerate(((False, None), (True, None), (False, 7), (True, 7))):
                fmt = (k + log_n) & 1
                want = b"".join(nu.expected_bytes(nu.transform(v, inverse, offset), fmt) for v in vals)
                got = c.fr_ntt(b"".join(nu.pack(v, fmt) for v in vals), log_n, 2, inverse, None if offset is None else nu.pack([offset], fmt), fmt)
                p = c.profile()
                ok = ok and got == want and p["window_bits"] <= cap
                passes.add(p["num_windows"])
            out["%%d,%%d" %% (cap, log_n)] = [ok, sorted(passes)]
print("RESULT " + json.dumps(out))
"""


def test_multi_pass_structure_test_build():
    """test build with MI_TEST_NTT_TILE_BITS = 1, 2, 3 (contexts created in a child process, so the environment is read): log_n 0..10, the
    four operations, batch 2, full comparison with Python; the profile shows one, two, three and at least four passes under every cap"""
    r = subprocess.run([sys.executable, "-c", _CHILD % {"root": ROOT, "here": HERE}], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    res = json.loads(line[7:])
    assert len(res) == 33
    for cap in (1, 2, 3):
        seen = set()
        for log_n in range(0, 11):
            ok, passes = res[f"{cap},{log_n}"]
            assert ok, (cap, log_n)
            assert passes == [max(1, -(-log_n // cap))], (cap, log_n, passes)   # the host form is never in place
            seen |= set(passes)
        assert {1, 2, 3} <= seen and max(seen) >= 4, (cap, seen)


@pytest.fixture(scope="module")
def ref_exe():
    return nu.host_exe("fr_ntt_ref")


def _random_words(n, seed, reduced=True):
    """n x 8 random 32-bit words as bytes; reduced: below 2^254 < r"""
    import numpy as np

    w = np.random.default_rng(seed).integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)
    if reduced:
        w[:, 7] &= 0x3FFFFFFF
    return w.tobytes()


def test_three_passes_against_cpp(ctx, ref_exe, tmp_path):
    """log_n = 2 levels + 1 (three passes, the middle pass with s > 1 and m > 1): the four operations in both formats, batch 2, out of place
    and in place (which takes an even number of passes), against the C++ reference"""
    levels = _levels(ctx)
    log_n = 2 * levels + 1
    data = _random_words(2 << log_n, 15, reduced=False)
    for k, (inverse, offset) in enumerate(MODES):
        for fmt in (0, 1):
            g = _offset_bytes(offset, fmt)
            want, _ = nu.run_ref(ref_exe, str(tmp_path), data, log_n, 2, inverse, g, fmt, threads=2)
            d_in, d_out = _dev(data), _dev(bytes(len(data)))
            ctx.fr_ntt_device(d_in.data_ptr(), log_n, 2, inverse, g, fmt, d_out.data_ptr())
            assert ctx.profile()["num_windows"] == 3
            got = d_out.cpu().numpy().tobytes()
            assert got == want, (inverse, offset, fmt, _first_diff(got, want))
            ctx.fr_ntt_device(d_in.data_ptr(), log_n, 2, inverse, g, fmt, d_in.data_ptr())
            assert ctx.profile()["num_windows"] == 4
            assert d_in.cpu().numpy().tobytes() == want, (inverse, offset, fmt, "in place")


def test_2_22_against_cpp(ctx, ref_exe, tmp_path):
    """2^22 elements (under 2 s of the C++ reference on one core), forward with the default coset, Montgomery form, host form"""
    log_n = 22
    data = _random_words(1 << log_n, 22)
    g = _offset_bytes(7, 1)
    want, secs = nu.run_ref(ref_exe, str(tmp_path), data, log_n, 1, False, g, 1)
    print(f"fr_ntt_ref 2^22: {secs:.2f} s")
    import numpy as np

    into = np.zeros(len(data), dtype=np.uint8)
    ctx.fr_ntt(data, log_n, 1, False, g, 1, into=into)
    assert into.tobytes() == want


@pytest.mark.parametrize("inverse", [False, True])
def test_largest_size_sparse(ctx, inverse):
    """2^26 elements, built and checked on the device: zero except five entries; 4096 random output rows plus rows 0, 1, n / 2, n - 1 against
    the closed form.  The size at which a byte offset no longer fits 31 bits.  Forward: canonical integers and a coset; inverse: Montgomery."""
    import torch

    log_n, n = 26, 1 << 26
    rnd = random.Random(26 + int(inverse))
    fmt = 1 if inverse else 0
    offset = None if inverse else 7
    entries = {j: rnd.randrange(1, R) for j in (0, 1, n // 2 + 1, n - 1, rnd.randrange(2, n - 1))}
    d_in = torch.zeros((n, 8), dtype=torch.int32, device="cuda")
    for j, v in entries.items():
        d_in[j] = torch.frombuffer(bytearray(nu.pack([v], fmt)), dtype=torch.int32).cuda()
    d_out = torch.empty((n, 8), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.fr_ntt_device(d_in.data_ptr(), log_n, 1, inverse, _offset_bytes(offset, fmt), fmt, d_out.data_ptr())
    p = ctx.profile()
    assert p["n"] == n and p["num_windows"] * p["window_bits"] >= log_n
    rows = [0, 1, n // 2, n - 1] + [rnd.randrange(n) for _ in range(4096)]
    got = d_out[torch.tensor(rows, device="cuda")].cpu().numpy().tobytes()
    want = nu.expected_bytes(nu.sparse_rows(entries, log_n, rows, inverse, offset), fmt)
    assert got == want, _first_diff(got, want)


def test_round_trips_2_20(ctx):
    """ifft(fft(a)) == a and coset_ifft(coset_fft(a)) == a on random reduced data at 2^20, in place, on the device"""
    import torch

    log_n = 20
    data = _random_words(1 << log_n, 20)
    for offset in (None, 7):
        g = _offset_bytes(offset, 1)
        d_a, d_b = _dev(data), _dev(data)
        ctx.fr_ntt_device(d_b.data_ptr(), log_n, 1, False, g, 1, d_b.data_ptr())
        assert not torch.equal(d_a, d_b)
        ctx.fr_ntt_device(d_b.data_ptr(), log_n, 1, True, g, 1, d_b.data_ptr())
        assert torch.equal(d_a, d_b), offset


def test_pipeline_into_msm_and_batch_mul(pkg, co):
    """evaluations on the device -> inverse NTT in place -> mi_msm_g1_device over resident bases, with no scalar on the host in between, equals
    the oracle's MSM over the Python coefficients; a coset forward transform feeds mi_g1_batch_mul_device the same way"""
    log_n, n = 10, 1 << 10
    rnd = random.Random(0x717E)
    evals = [rnd.randrange(R) for _ in range(n)]
    coeffs = nu.ifft(evals)
    bases = co.gen_bases("g1", 0x717F, n, 4)
    with pkg.Context([0]) as c:
        c.set_bases("g1", bases, n)
        d = _dev(nu.pack(evals, 1))
        c.fr_ntt_device(d.data_ptr(), log_n, 1, True, None, 1, d.data_ptr())
        got = c.msm_device("g1", d.data_ptr(), n, pkg.SCALAR_MONTGOMERY)
        want = co.msm("g1", bases, nu.pack(coeffs, 0), n, 0, 4)
        assert co.to_affine("g1", got) == co.to_affine("g1", want)
        m = 64   # the oracle multiplies the generator one scalar at a time (12 ms each)
        sub = coeffs[:m]
        d = _dev(nu.pack(sub, 1))
        c.fr_ntt_device(d.data_ptr(), 6, 1, False, nu.pack([7], 1), 1, d.data_ptr())
        d_pts = _dev(bytes(96 * m))
        c.batch_mul_device("g1", co.mul_gen("g1", 1), d.data_ptr(), m, pkg.SCALAR_MONTGOMERY, d_pts.data_ptr())
        want = b"".join(co.mul_gen("g1", s) if s else bytes(96) for s in nu.coset_fft(sub, 7))
        assert d_pts.cpu().numpy().tobytes() == want


def test_arguments_and_cache(pkg):
    """every MI_E_INVALID case; a second call of the same size builds nothing; the coset offset keys the cache"""
    import ctypes as C

    rnd = random.Random(9)
    vals = [rnd.randrange(R) for _ in range(16)]
    data = nu.pack(vals, 1)
    with pkg.Context([0]) as c:
        L, h = c._L, c._h
        out = C.create_string_buffer(len(data))
        d_in, d_out = _dev(data), _dev(data)
        g7 = nu.pack([7], 1)
        bad_host = [
            (None, 4, 1, 0, None, 1, out), (data, 4, 1, 0, None, 1, None),       # NULL data
            (data, 4, 1, 0, None, 2, out), (data, 4, 1, 2, None, 1, out), (data, 4, 1, -1, None, 1, out),   # scalar_fmt, inverse
            (data, 4, 1, 0, bytes(32), 1, out), (data, 4, 1, 0, nu.pack_raw([R]), 0, out), (data, 4, 1, 1, nu.pack_raw([2 * R]), 1, out),   # zero offsets
            (data, 4, 0, 0, None, 1, out), (data, 27, 1, 0, None, 1, out), (data, 4, 1 << 60, 0, None, 1, out), (data, 26, 1 << 40, 0, None, 1, out)]
        for a in bad_host:
            assert L.mi_fr_ntt(h, *a) == -1, a[1:6]
        assert out.raw == bytes(len(data))
        p_in, p_out = d_in.data_ptr(), d_out.data_ptr()
        for a in ((p_in, 4, 1, 0, None, 1, p_in + 32), (p_in + 8, 4, 1, 0, None, 1, p_out), (4096, 4, 1, 0, None, 1, p_out), (p_in, 4, 1, 0, None, 1, 4096),
                  (0, 4, 1, 0, None, 1, p_out), (p_in, 4, 1, 0, None, 3, p_out)):
            assert L.mi_fr_ntt_device(h, C.c_void_p(a[0]), *a[1:6], C.c_void_p(a[6])) == -1, a
        for a in ((3, p_in, p_out, 16, 1, p_out), (-1, p_in, p_out, 16, 1, p_out), (0, p_in, p_out, 16, 2, p_out), (0, 0, p_out, 16, 1, p_out),
                  (0, p_in, p_out, 16, 1, 0), (0, p_in, p_out, 15, 1, p_out + 32), (0, p_in + 4, p_out, 15, 1, p_out), (0, 4096, p_out, 16, 1, p_out)):
            assert L.mi_fr_vec_op_device(h, a[0], C.c_void_p(a[1]), C.c_void_p(a[2]), a[3], a[4], C.c_void_p(a[5])) == -1, a
        assert L.mi_fr_vec_op_device(h, 0, None, None, 0, 1, None) == 0
        assert d_in.cpu().numpy().tobytes() == data and d_out.cpu().numpy().tobytes() == data   # nothing was touched
        # tables: built on the first call of a (size, direction, offset), resident afterwards
        assert c.fr_ntt(data, 4, 1, False, None, 1) == nu.expected_bytes(nu.fft(vals), 1) and c.profile()["ingest_ms"] > 0
        assert c.fr_ntt(data, 4, 1, False, None, 1) == nu.expected_bytes(nu.fft(vals), 1) and c.profile()["ingest_ms"] == 0
        assert c.fr_ntt(data, 4, 1, True, None, 1) == nu.expected_bytes(nu.ifft(vals), 1) and c.profile()["ingest_ms"] > 0
        assert c.fr_ntt(data, 4, 1, False, g7, 1) == nu.expected_bytes(nu.coset_fft(vals, 7), 1) and c.profile()["ingest_ms"] > 0
        assert c.fr_ntt(data, 4, 1, False, g7, 1) == nu.expected_bytes(nu.coset_fft(vals, 7), 1) and c.profile()["ingest_ms"] == 0
        g = rnd.randrange(2, R)
        got = c.fr_ntt(data, 4, 1, False, nu.pack([g], 1), 1)
        assert got == nu.expected_bytes(nu.coset_fft(vals, g), 1) != nu.expected_bytes(nu.coset_fft(vals, 7), 1) and c.profile()["ingest_ms"] > 0
        assert c.fr_ntt(data, 4, 1, False, g7, 1) == nu.expected_bytes(nu.coset_fft(vals, 7), 1) and c.profile()["ingest_ms"] == 0
        # the same offset given in the other format is the same table; more sizes than the context keeps evict the oldest and stay correct
        assert c.fr_ntt(nu.pack(vals, 0), 4, 1, False, nu.pack([7], 0), 0) == nu.expected_bytes(nu.coset_fft(vals, 7), 0) and c.profile()["ingest_ms"] == 0
        for log_n in range(0, 10):
            v = [rnd.randrange(R) for _ in range(1 << log_n)]
            assert c.fr_ntt(nu.pack(v, 1), log_n, 1, False, None, 1) == nu.expected_bytes(nu.fft(v), 1)
        assert c.fr_ntt(data, 4, 1, False, g7, 1) == nu.expected_bytes(nu.coset_fft(vals, 7), 1) and c.profile()["ingest_ms"] > 0


def test_python_mirror(pkg):
    """Radix2EvaluationDomain of msm.py: zero padding of a shorter input, the default offset 7, Montgomery by default"""
    rnd = random.Random(12)
    vals = [rnd.randrange(R) for _ in range(11)]
    D = pkg.Radix2EvaluationDomain.new(11)
    assert D.size == 16
    padded = vals + [0] * 5
    assert D.fft(nu.pack(vals, 1)) == nu.expected_bytes(nu.fft(padded), 1)
    assert D.ifft(nu.pack(padded, 1)) == nu.expected_bytes(nu.ifft(padded), 1)
    assert D.coset_fft(nu.pack(vals, 1)) == nu.expected_bytes(nu.coset_fft(padded, 7), 1)
    assert D.coset_ifft(nu.pack(padded, 0), 5, scalar_fmt=pkg.SCALAR_CANONICAL) == nu.expected_bytes(nu.coset_ifft(padded, 5), 0)
    assert D.ifft(D.fft(nu.pack(vals, 1))) == nu.pack(padded, 1)
