"""GPU tests of the MSM's third stage on constructed buckets (tests/msm_reduce_util.py): k_merge, k_reduce_coop, k_reduce_serial and every
level of k_combine (csrc/curve_kernels.cuh), each with the geometry FORCED through the test build's plan switches (csrc/msm_sort.hip:
MI_TEST_COOP_L, MI_TEST_SERIAL_MIN_BUCKETS, MI_TEST_SERIAL_L) and confirmed through test_plan().

Every base is a known multiple of the generator and every scalar m 2^(c w) has one digit, so every bucket of every window is dictated and
every window sum is (sum m k mod r) G, independent of any pipeline.  msm_device_windows hands the window sums back before the Horner fold:
each window of a call is one reduction checked on its own, byte for byte on the canonical affine encoding; an expected infinity must come
back as all-zero bytes.  tests/test_msm_reduce_cpu.py proves on the CPU which operand classes of the complete addition these patterns put
into which step of which kernel."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import msm_digits_util as du  # noqa: E402
import msm_reduce_util as ru  # noqa: E402

pytestmark = pytest.mark.gpu

GROUPS = ["g1", "g2"]
SWITCHES = ("MI_TEST_COOP_L", "MI_TEST_SERIAL_MIN_BUCKETS", "MI_TEST_SERIAL_L")


def _sizes(group):
    return (96, 144) if group == "g1" else (192, 288)


def _point(co, group, k):
    """k G as canonical affine bytes, infinity = zeros"""
    return ru.mul_gen(co, group, k) if k % ru.R else bytes(_sizes(group)[0])


def _window_sums(pkg, co, cx, group, c, b, fold=False, windows=None):
    """one call of msm_device_windows and one of msm over the built vectors, both held against the closed form -> the window sums (affine)"""
    import torch

    aff, jac = _sizes(group)
    W = du.windows(c, fold) if windows is None else windows
    d = torch.frombuffer(bytearray(b.scalars), dtype=torch.uint8).cuda()
    out = torch.full((pkg.MAX_WINDOWS * jac,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert cx.msm_device_windows(group, d.data_ptr(), b.n, pkg.SCALAR_CANONICAL, out.data_ptr()) == (c, W)
    torch.cuda.synchronize()
    raw = out.cpu().numpy().tobytes()
    expected = b.expected if windows is None else [b.total]
    got = []
    for w in range(W):
        one = raw[w * jac:(w + 1) * jac]
        if expected[w] == 0:
            assert one == bytes(jac), (group, c, w, "infinity is the all-zero point")
        got.append(co.to_affine(group, one))
        assert got[w] == _point(co, group, expected[w]), (group, c, w)
    assert co.to_affine(group, cx.msm(group, None, b.scalars, b.n, pkg.SCALAR_CANONICAL)) == _point(co, group, b.total), (group, c)
    p = cx.profile()
    assert p["window_bits"] == c and p["n"] == b.n
    return got


def _clear(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize("group,L,c", [(g, L, c) for g in GROUPS for L, c in ru.COOP_CASES[g]])
def test_reduce_coop_forced_L(pkg, co, tctx, monkeypatch, group, L, c):
    """k_reduce_coop<QuadG1> (16 logical lanes) / <PairG2> (32) with L buckets per lane pinned, and the k_combine levels behind it
    (QuadG1 / OctG2): at least two chunks per window at the smallest such c — a ragged last chunk whenever L is no power of two —, one
    chunk exactly (k_combine's cpw_in == 1 path), and hundreds of chunks (several combine levels).  Every window carries another pattern."""
    g = ru.geo_coop(group, c, L)
    _clear(monkeypatch)
    monkeypatch.setenv("MI_TEST_COOP_L", str(L))
    tctx.set_window_bits(c)
    try:
        for call in ru.place(ru.patterns(g), c):
            b = ru.build(co, group, c, call)
            plan = pkg.test_plan(b.n, c, group, False)
            assert (plan["c"], plan["coop_L"], plan["chunk_buckets"], plan["chunks_per_win"], plan["serial_reduce"]) == (c, L, g.K, g.cpw, 0), plan
            tctx.set_bases(group, b.bases, b.n)
            _window_sums(pkg, co, tctx, group, c, b)
    finally:
        tctx.set_window_bits(0)


@pytest.mark.parametrize("L,c", ru.SERIAL_CASES)
def test_reduce_serial_forced_L(pkg, co, tctx, monkeypatch, L, c):
    """k_reduce_serial (G1; production reaches it from 2^21 buckets on) with one lane per L buckets: L = 1 (no chain), ragged last lanes,
    waves that span windows, idle lanes in the last wave (c = 7: 37 windows of 64 buckets).  The same input then goes through
    k_reduce_coop, and the two implementations' window sums must agree."""
    g = ru.geo_serial(c, L)
    tctx.set_window_bits(c)
    try:
        for call in ru.place(ru.patterns(g), c):
            b = ru.build(co, "g1", c, call)
            _clear(monkeypatch)
            monkeypatch.setenv("MI_TEST_SERIAL_MIN_BUCKETS", "1")
            monkeypatch.setenv("MI_TEST_SERIAL_L", str(L))
            plan = pkg.test_plan(b.n, c, "g1", False)
            assert (plan["c"], plan["serial_reduce"], plan["serial_L"], plan["chunks_per_win"], plan["coop_L"]) == (c, 1, L, g.cpw, 0), plan
            assert plan["nchunks"] == g.cpw * du.windows(c, False)
            tctx.set_bases("g1", b.bases, b.n)
            serial = _window_sums(pkg, co, tctx, "g1", c, b)
            _clear(monkeypatch)
            plan = pkg.test_plan(b.n, c, "g1", False)
            assert plan["serial_reduce"] == 0 and plan["coop_L"] >= 1
            assert _window_sums(pkg, co, tctx, "g1", c, b) == serial
    finally:
        tctx.set_window_bits(0)


@pytest.mark.parametrize("group", GROUPS)
def test_merge_of_split_buckets(pkg, co, tctx, monkeypatch, group):
    """k_merge<QuadG1> / <OctG2>: buckets of window 0 and of the top window filled beyond T = 2^logT entries, 3 / 4 / 5 / 16 / 17 items
    (one, two and three levels of fan-in 4; the room / m arithmetic at the boundaries), with equal item sums, items that are infinity,
    and a bucket that merges to infinity."""
    _clear(monkeypatch)
    c = 10                                        # 512 buckets per window: the mean load stays small and the plan keeps T = 32, S = 16
    top = du.windows(c, False) - 1
    assert ru.max_magnitude(c, top) >= len(ru.MERGE_KINDS)
    tctx.set_window_bits(c)
    try:
        logT = 5
        for count in ru.merge_counts(logT):
            low = {m: ru.merge_entries(kind, count, logT) for m, kind in zip((3, 17, 18, 256, 511, 512), ru.MERGE_KINDS)}
            high = {m + 1: ru.merge_entries(kind, count, logT) for m, kind in enumerate(ru.MERGE_KINDS)}
            b = ru.build(co, group, c, [(0, low), (top, high)])
            plan = pkg.test_plan(b.n, c, group, False)
            assert plan["logT"] == logT and plan["serial_reduce"] == 0, plan       # the item geometry the entries were counted for
            tctx.set_bases(group, b.bases, b.n)
            _window_sums(pkg, co, tctx, group, c, b)
            assert tctx.profile()["max_items_per_bucket"] == count
    finally:
        tctx.set_window_bits(0)


@pytest.mark.parametrize("group", GROUPS)
def test_validated_set_folds_signs(pkg, co, tctx, monkeypatch, group):
    """a validated resident set: every scalar is r - m 2^(c w) > (r - 1) / 2, the library recodes m 2^(c w) with the signs inverted; the
    bases are the negatives, so every bucket — and every window sum — is what the pattern says"""
    c, L = 8, 3
    g = ru.geo_coop(group, c, L)
    _clear(monkeypatch)
    monkeypatch.setenv("MI_TEST_COOP_L", str(L))
    tctx.set_window_bits(c)
    try:
        call = ru.place(ru.patterns(g), c, fold=True)[0]
        b = ru.build(co, group, c, call, fold=True)
        assert all(int.from_bytes(b.scalars[32 * i:32 * i + 32], "little") > (ru.R - 1) // 2 for i in range(b.n))
        plan = pkg.test_plan(b.n, c, group, False, 0, True)
        assert (plan["coop_L"], plan["chunks_per_win"], plan["nwin"]) == (L, g.cpw, du.windows(c, True)), plan
        tctx.set_bases(group, b.bases, b.n)
        assert tctx.validate_bases(group) == 0
        _window_sums(pkg, co, tctx, group, c, b, fold=True)
    finally:
        tctx.set_window_bits(0)


@pytest.mark.parametrize("group", GROUPS)
def test_precomputed_tables_share_one_bucket_set(pkg, co, monkeypatch, group):
    """set_bases_precomputed: the entries of every window meet in ONE bucket set (bwin == 1), a base of window w enters as 2^(c w) times
    itself; there are no per-window sums, the one sum is the result"""
    c = 8
    _clear(monkeypatch)
    with pkg.Context([0], test_hooks=True) as cp:
        g = ru.geo_coop(group, c, 2)
        call = ru.place(ru.patterns(g), c)[0]
        b = ru.build(co, group, c, call)
        assert b.total != 0
        plan = pkg.test_plan(b.n, c, group, True, b.n)
        assert plan["c"] == c and plan["bwin"] == 1 and plan["serial_reduce"] == 0, plan
        cp.set_bases_precomputed(group, b.bases, b.n, c)
        _window_sums(pkg, co, cp, group, c, b, windows=1)
