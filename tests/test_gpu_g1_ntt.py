"""GPU tests of the NTT over G1 points (mi_g1_ntt, mi_g1_ntt_device).  Every comparison is of exact output bytes: against the definition
computed by the C oracle (one naive MSM per output row), against the closed form for a powers-of-tau input, and — for inputs of known
discrete logarithm — against the scalar transform of the logarithms (tests/ntt_util.py) carried back to the curve by mi_g1_batch_mul, with
sampled rows from the oracle's generator multiplication."""
import ctypes as C
import os
import random
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import g1_ntt_util as gu  # noqa: E402
import ntt_util as nu  # noqa: E402

pytestmark = pytest.mark.gpu
R, AFF, INF = gu.R, gu.AFF, gu.INF


def _dev(data: bytes):
    import torch

    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return t


def _bytes(t) -> bytes:
    return t.cpu().numpy().tobytes()


def _first_diff(got, want):
    bad = [i for i in range(len(want) // AFF) if got[AFF * i:AFF * i + AFF] != want[AFF * i:AFF * i + AFF]]
    return f"{len(bad)} of {len(want) // AFF} points differ, first at {bad[:8]}"


def _gen(co) -> bytes:
    return co.mul_gen("g1", 1)


def _points_of(ctx, co, logs) -> bytes:
    """[k] G for every k (0 -> the all-zero point), by the fixed-base multiplication"""
    return ctx.batch_mul("g1", _gen(co), gu.pack_scalars(k % R for k in logs), 0)


def _sample_rows(n: int, rnd, count: int = 32):
    rows = {0, 1 % n, n // 2, n - 1}
    while len(rows) < min(count, n):
        rows.add(rnd.randrange(n))
    return sorted(rows)


def _check_by_logs(ctx, co, logs, log_n, inverse, got, rnd, what):
    """got == [c_k] G for c = the scalar transform of the logarithms: every row through batch_mul, sampled rows through the oracle"""
    want_logs = nu.transform([k % R for k in logs], inverse)
    want = _points_of(ctx, co, want_logs)
    assert got == want, (what, log_n, inverse, _first_diff(got, want))
    for k in _sample_rows(1 << log_n, rnd, 8):
        assert gu.point(got, k) == (co.mul_gen("g1", want_logs[k]) if want_logs[k] else INF), (what, log_n, inverse, k)
    return want_logs


@pytest.mark.parametrize("inverse", [False, True])
def test_definition(ctx, co, inverse):
    """log_n 0..6 on random points of the oracle: no level, one trivial level, the first non-trivial twiddle, a partial workgroup, both
    parities of the ping-pong; expected = one naive MSM of the oracle per output row with the scalars w^(+-jk) (times 1 / n)"""
    for log_n in range(0, 7):
        n = 1 << log_n
        pts = co.gen_bases("g1", 900 + log_n, n)
        want = gu.definition(co, pts, log_n, inverse)
        got = ctx.g1_ntt(pts, log_n, inverse)
        assert got == want, (log_n, _first_diff(got, want))
        p = ctx.profile()
        assert p["num_windows"] == log_n and p["n"] == n


_TAU = 0x2B5C0DE5EED0F7A1C0FFEE1234567890ABCDEF0FEDCBA98765432100F1E2D3C4 % R


@pytest.mark.parametrize("log_n", [7, 8, 10, 12, 14])
def test_closed_form(ctx, co, log_n):
    """P_j = [tau^j] G: forward out[k] = [(tau^n - 1) / (tau w^k - 1)] G, inverse out[k] = [(tau^n - 1) w^k / (n (tau - w^k))] G — the
    Lagrange-basis SRS.  Every row against batch_mul on the closed-form scalars, 32 sampled rows (0, 1, n / 2, n - 1 among them) against
    the oracle's generator multiplication."""
    n = 1 << log_n
    rnd = random.Random(log_n)
    pw = gu.powers(_TAU, n)
    srs = ctx.batch_mul("g1", _gen(co), gu.pack_scalars(pw), 0)
    for j in _sample_rows(n, rnd, 16):
        assert gu.point(srs, j) == co.mul_gen("g1", pw[j]), j
    for inverse in (False, True):
        sc = gu.closed_form_scalars(_TAU, log_n, inverse)
        want = ctx.batch_mul("g1", _gen(co), gu.pack_scalars(sc), 0)
        got = ctx.g1_ntt(srs, log_n, inverse)
        assert got == want, (log_n, inverse, _first_diff(got, want))
        for k in _sample_rows(n, rnd, 32):
            assert gu.point(got, k) == co.mul_gen("g1", sc[k]), (log_n, inverse, k)


@pytest.mark.parametrize("log_n", [6, 9])
@pytest.mark.parametrize("inverse", [False, True])
def test_structured_inputs(ctx, co, log_n, inverse):
    """all infinity; one point among infinities; the same point everywhere (every first-level butterfly is a doubling or a cancellation,
    every later level meets infinity); P_(j + n/2) = -P_j; random points with every third one at infinity"""
    n = 1 << log_n
    rnd = random.Random(31 * log_n + int(inverse))
    w = nu.omega(log_n, inverse)
    scale = pow(n, -1, R) if inverse else 1
    assert ctx.g1_ntt(INF * n, log_n, inverse) == INF * n
    a = rnd.randrange(1, R)
    pa = co.mul_gen("g1", a)
    for j in (0, 1, n - 1):
        logs = [0] * n
        logs[j] = a
        got = ctx.g1_ntt(INF * j + pa + INF * (n - 1 - j), log_n, inverse)
        want_logs = _check_by_logs(ctx, co, logs, log_n, inverse, got, rnd, ("single", j))
        assert want_logs == [a * scale * pow(w, j * k, R) % R for k in range(n)]   # out[k] = [w^(jk)] P (times 1 / n)
    got = ctx.g1_ntt(pa * n, log_n, inverse)
    assert got == co.mul_gen("g1", a if inverse else a * n % R) + INF * (n - 1), ("same point", _first_diff(got, pa + INF * (n - 1)))
    half = [rnd.randrange(1, R) for _ in range(n // 2)]
    logs = half + [R - k for k in half]
    got = ctx.g1_ntt(_points_of(ctx, co, logs), log_n, inverse)
    _check_by_logs(ctx, co, logs, log_n, inverse, got, rnd, "antisymmetric")
    assert all(gu.point(got, k) == INF for k in range(0, n, 2)) and all(gu.point(got, k) != INF for k in range(1, n, 2))
    logs = [0 if j % 3 == 0 else rnd.randrange(1, R) for j in range(n)]
    pts = _points_of(ctx, co, logs)
    assert all((gu.point(pts, j) == INF) == (j % 3 == 0) for j in range(n))
    _check_by_logs(ctx, co, logs, log_n, inverse, ctx.g1_ntt(pts, log_n, inverse), rnd, "every third at infinity")


def test_forms(pkg, ctx, co, tmp_path):
    """log_n = 10: inverse(forward(x)) == x; the device form equals the host form; in place equals out of place; two calls of different
    size and direction on one context give the bytes fresh contexts give (the tables are reused, not confused)"""
    log_n, n = 10, 1 << 10
    pts = co.gen_bases("g1", 0x610, n, 4)
    fwd = ctx.g1_ntt(pts, log_n, False)
    assert fwd != pts and ctx.g1_ntt(fwd, log_n, True) == pts
    inv = ctx.g1_ntt(pts, log_n, True)
    for inverse, want in ((False, fwd), (True, inv)):
        d_in, d_out = _dev(pts), _dev(bytes([0x5A]) * len(pts))
        ctx.g1_ntt_device(d_in.data_ptr(), log_n, inverse, d_out.data_ptr())
        assert _bytes(d_out) == want and _bytes(d_in) == pts, ("device", inverse)
        p = ctx.profile()
        assert p["num_windows"] == log_n and p["n"] == n and p["h2d_ms"] == 0 and p["accumulate_ms"] > 0 and p["reduce_ms"] > 0
        ctx.g1_ntt_device(d_in.data_ptr(), log_n, inverse, d_in.data_ptr())
        assert _bytes(d_in) == want, ("in place", inverse)
    small = pts[:AFF << 7]
    with pkg.Context([0]) as c:
        a = c.g1_ntt(small, 7, True)
        assert c.profile()["ingest_ms"] > 0
        b = c.g1_ntt(pts, log_n, False)
        a2 = c.g1_ntt(small, 7, True)
        assert c.profile()["ingest_ms"] == 0
    with pkg.Context([0]) as c:
        assert c.g1_ntt(pts, log_n, False) == b == fwd
    with pkg.Context([0]) as c:
        assert c.g1_ntt(small, 7, True) == a == a2
    # log_n = 0, device form: the point is copied, or stays where it is
    one = gu.point(pts, 5)
    d_in, d_out = _dev(one), _dev(bytes([0x5A]) * AFF)
    for inverse in (False, True):
        ctx.g1_ntt_device(d_in.data_ptr(), 0, inverse, d_out.data_ptr())
        assert _bytes(d_out) == one and _bytes(d_in) == one and ctx.profile()["num_windows"] == 0
        ctx.g1_ntt_device(d_in.data_ptr(), 0, inverse, d_in.data_ptr())
        assert _bytes(d_in) == one
        d_out.fill_(0x5A)
    # the C++ mirror: Radix2EvaluationDomain::fft / ifft over std::vector<G1Affine>, built against the C-ABI library, run as a child process
    for name, content in (("in", small), ("fft", ctx.g1_ntt(small, 7, False)), ("ifft", a)):
        (tmp_path / f"{name}.bin").write_bytes(content)
    exe = os.path.join(HERE, "host", "g1_ntt_mirror_test")
    lib = os.path.join(ROOT, "ark-blst_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "host", "g1_ntt_mirror_test.cpp"), "-L" + lib, "-larkblst_amd",
                           "-Wl,-rpath," + lib])
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "g1 fft OK" in out.stdout, out.stdout + out.stderr


def test_chunking_test_build(tctx, ctx, co):
    """the host form's results leave in chunks (normalisation level 0 and the copy per chunk).  Test build, log_n = 10, the chunk forced to
    2^7 and to 2^6 through MI_TEST_G1NTT_CHUNK: eight chunks, the bytes of the default (one chunk) and of the product build"""
    log_n, n = 10, 1 << 10
    pts = bytearray(co.gen_bases("g1", 0xC4, n, 4))
    for j in (0, 127, 128, 500, n - 1):   # infinity at the edges of chunks: the tree skips it, the output is all-zero
        pts[AFF * j:AFF * (j + 1)] = INF
    pts = bytes(pts)
    assert "MI_TEST_G1NTT_CHUNK" not in os.environ
    for inverse in (False, True):
        want = ctx.g1_ntt(pts, log_n, inverse)
        assert tctx.g1_ntt(pts, log_n, inverse) == want and tctx.profile()["work_items"] == 1
        try:
            for chunk, chunks in ((128, 8), (64, 8), (256, 4)):
                os.environ["MI_TEST_G1NTT_CHUNK"] = str(chunk)
                got = tctx.g1_ntt(pts, log_n, inverse)
                assert got == want, (inverse, chunk, _first_diff(got, want))
                assert tctx.profile()["work_items"] == chunks, (chunk, tctx.profile()["work_items"])
                d_in, d_out = _dev(pts), _dev(bytes(len(pts)))
                tctx.g1_ntt_device(d_in.data_ptr(), log_n, inverse, d_out.data_ptr())   # nothing crosses PCIe: one chunk whatever the switch says
                assert _bytes(d_out) == want and tctx.profile()["work_items"] == 1
                os.environ["MI_TEST_G1NTT_CHUNK"] = "128"
                assert ctx.g1_ntt(pts, log_n, inverse) == want and ctx.profile()["work_items"] == 1   # the product build does not read it
        finally:
            os.environ.pop("MI_TEST_G1NTT_CHUNK", None)


def test_host_form_in_chunks_by_default(ctx, co):
    """2^17 points, where the host form's results leave in two chunks without any switch: equal to the device form, sampled rows against the
    closed form of the powers-of-tau input"""
    log_n, n = 17, 1 << 17
    rnd = random.Random(17)
    srs = ctx.batch_mul("g1", _gen(co), gu.pack_scalars(gu.powers(_TAU, n)), 0)
    got = ctx.g1_ntt(srs, log_n, True)
    assert ctx.profile()["work_items"] == 2 and ctx.profile()["h2d_ms"] > 0
    d_in = _dev(srs)
    ctx.g1_ntt_device(d_in.data_ptr(), log_n, True, d_in.data_ptr())
    assert _bytes(d_in) == got
    sc = gu.closed_form_scalars(_TAU, log_n, True)
    for k in _sample_rows(n, rnd, 32) + [n // 2 - 1, n // 2 + 1]:
        assert gu.point(got, k) == co.mul_gen("g1", sc[k]), k


def test_end_to_end_lagrange_commitment(ctx, co):
    """n = 2^10, nothing on the host between the steps: monomial SRS by batch_mul_device, Lagrange SRS by g1_ntt_device(inverse); committing
    to evaluations over the Lagrange bases equals committing to fr_ntt_device(inverse) of them over the monomial bases equals [p(tau)] G"""
    log_n, n = 10, 1 << 10
    rnd = random.Random(0xE2E)
    pw = gu.powers(_TAU, n)
    d_pw = _dev(gu.pack_scalars(pw))
    d_srs, d_lag = _dev(bytes(AFF * n)), _dev(bytes(AFF * n))
    ctx.batch_mul_device("g1", _gen(co), d_pw.data_ptr(), n, 0, d_srs.data_ptr())
    ctx.g1_ntt_device(d_srs.data_ptr(), log_n, True, d_lag.data_ptr())
    evals = [rnd.randrange(R) for _ in range(n)]
    d_e = _dev(gu.pack_scalars(evals))
    ctx.set_bases_device("g1", d_lag.data_ptr(), n)
    by_lagrange = co.to_affine("g1", ctx.msm_device("g1", d_e.data_ptr(), n, 0))
    d_c = _dev(bytes(32 * n))
    ctx.fr_ntt_device(d_e.data_ptr(), log_n, 1, True, None, 0, d_c.data_ptr())
    ctx.set_bases_device("g1", d_srs.data_ptr(), n)
    by_monomial = co.to_affine("g1", ctx.msm_device("g1", d_c.data_ptr(), n, 0))
    coeffs = nu.ifft(evals)
    assert _bytes(d_c) == gu.pack_scalars(coeffs)
    value = sum(c * t for c, t in zip(coeffs, pw)) % R
    assert by_lagrange == by_monomial == co.mul_gen("g1", value)


def test_arguments(pkg, co):
    """every MI_E_INVALID case of the header, refused before anything is touched; log_n = 25 is refused without an allocation"""
    import torch

    log_n, n = 4, 16
    pts = co.gen_bases("g1", 0xA46, n)
    with pkg.Context([0]) as c:
        L, h = c._L, c._h
        out = C.create_string_buffer(len(pts))
        d_in, d_out = _dev(pts), _dev(pts)
        p_in, p_out = d_in.data_ptr(), d_out.data_ptr()
        for a in ((None, log_n, 0, out), (pts, log_n, 0, None), (pts, log_n, 2, out), (pts, log_n, -1, out), (pts, 25, 0, out), (pts, 1 << 31, 1, out)):
            assert L.mi_g1_ntt(h, *a) == -1, a[1:3]
        assert out.raw == bytes(len(pts))
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        assert L.mi_g1_ntt_device(h, C.c_void_p(p_in), 25, 0, C.c_void_p(p_out)) == -1
        assert L.mi_g1_ntt(h, pts, 25, 1, out) == -1
        assert torch.cuda.mem_get_info()[0] == free0
        for a in ((0, log_n, 0, p_out), (p_in, log_n, 0, 0), (p_in, log_n, 3, p_out), (p_in, 25, 0, p_out),
                  (p_in, log_n, 0, p_in + AFF), (p_in, 3, 0, p_in + 7 * AFF), (p_in + 8, 3, 0, p_out), (p_in, 3, 0, p_out + 8),   # overlap, alignment
                  (4096, log_n, 0, p_out), (p_in, log_n, 0, 4096)):                                                                # not device memory
            assert L.mi_g1_ntt_device(h, C.c_void_p(a[0]), a[1], a[2], C.c_void_p(a[3])) == -1, a
        host = torch.zeros(len(pts), dtype=torch.uint8)
        assert L.mi_g1_ntt_device(h, C.c_void_p(host.data_ptr()), log_n, 0, C.c_void_p(p_out)) == -1
        assert _bytes(d_in) == pts and _bytes(d_out) == pts and out.raw == bytes(len(pts))   # nothing was touched
        assert c.g1_ntt(pts, log_n, False) == gu.definition(co, pts, log_n, False)           # and the context still works
    with pkg.Context([0, 0]) as c2:   # two devices: the device form is refused, the host form runs on the first
        assert c2._L.mi_g1_ntt_device(c2._h, C.c_void_p(p_in), log_n, 0, C.c_void_p(p_out)) == -1 and _bytes(d_out) == pts
        assert c2.g1_ntt(pts, log_n, True) == gu.definition(co, pts, log_n, True)
