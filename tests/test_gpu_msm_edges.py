"""GPU tests of the MSM on inputs random data never produces: the edges of the signed-digit recoding (load_scalar / for_each_digit_static,
csrc/kernels_common.cuh, in all four sort kernels of csrc/sort_kernels.cuh) and the exceptional pairs of the accumulate kernels
(k_accumulate / k_accumulate_g2_coop, csrc/curve_kernels.cuh).  Every comparison is byte equality on the canonical affine encoding.

Which kernel a call reaches follows from its size and window size (run_sort, csrc/msm_sort.hip) and shows in the asserted profile fields:
  n = 300            k_coarse does the count and the scatter pass (c <= 16); k_coarseA for c >= 17 (three-level sort)
  n = 4096 + 37      k_coarse_staged scatters for c <= 16 (one full tile and a ragged one)
  window_groups > 1  the later groups of a pipelined call sort with k_coarse_staged_co (c <= 16), carries cross the group boundaries
  validated set      sign fold: num_windows drops by one at c = 15 and c = 17
  precomputed set    every window feeds one bucket set: the g.shared path of k_coarse, for every c"""
import os
import random
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import msm_digits_util as du  # noqa: E402

pytestmark = pytest.mark.gpu

GROUPS = ["g1", "g2"]
N_SMALL, N_BIG = 300, 4096 + 37
SEED_B, SEED_S = 0xED6E0, 0xED6E1
_CACHE = {}


def _curve(o, group):
    return (o.F1, 96) if group == "g1" else (o.F2, 192)


def _canon(co, group, jac):
    return co.to_affine(group, jac)


def _bases(co, group):
    """N_BIG points k_i G of the C oracle's generator (the first N_SMALL of them are the small set), once per group"""
    if ("bases", group) not in _CACHE:
        _CACHE["bases", group] = co.gen_bases(group, SEED_B, N_BIG, 8)
    return _CACHE["bases", group]


def _mul(o, group, base_bytes, s):
    """big-int oracle: (s mod r) * base as canonical affine bytes, shared by every test of the module"""
    F, aff = _curve(o, group)
    key = ("mul", group, base_bytes, s % o.R_ORDER)
    if key not in _CACHE:
        q = o.scalar_mul(F, o.affine_from_bytes(F, base_bytes), s % o.R_ORDER)
        _CACHE[key] = o.affine_to_bytes(F, q) if q is not o.INF else bytes(aff)
    return _CACHE[key]


def _edge_vector(co, o, c, n):
    """(raw scalars, the same reduced modulo r): the special scalars of window size c spread over n positions — the first and the last
    one included, and again over the last 37 (the ragged tile of N_BIG) — between the C oracle's random scalars"""
    r = o.R_ORDER
    special = du.special_scalars(c, r)
    assert len(special) <= n - 37
    fill = co.gen_scalars(SEED_S + c, n)
    vals = [int.from_bytes(fill[32 * i:32 * i + 32], "little") for i in range(n)]
    for k, v in enumerate(special):
        vals[k * (n - 38) // (len(special) - 1)] = v
    for k in range(37):
        vals[n - 1 - k] = special[-1 - k % len(special)]        # the constructed digit patterns and the top windows' edges, in the last tile
    assert vals[0] == special[0] and vals[n - 1] == special[-1] and all(vals.count(v) >= 1 for v in special)
    return du.scalar_bytes(vals), du.scalar_bytes([v % r for v in vals])


def _single_scalars(o, c):
    """the scalars of the one-point calls: the group-order edges, the fold threshold and the constructed digit patterns (all ties, all
    first-negative, a carry through every window, ...) with their fold images"""
    r = o.R_ORDER
    special = du.special_scalars(c, r)
    return special[3:15] + special[-13:]


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("c", du.C_ALL)
def test_digit_recoding_edges(pkg, co, o, group, c):
    """The special scalars of msm_digits_util (raw digits at 2^(c-1), 2^(c-1) + 1 and 2^c, carries through every window, the carry-only
    top window of c = 15 / 17, the fold threshold, values >= r) through every way an MSM can be called, against the closed form
    (sum s_i k_i) G over the values reduced in Python — which involves no Pippenger and no recoding."""
    import torch

    F, aff = _curve(o, group)
    bases = _bases(co, group)
    w_plain, w_fold = du.windows(c, False), du.windows(c, True)
    assert w_plain - w_fold == (1 if c in (15, 17) else 0)
    vec = {}
    for n in (N_SMALL, N_BIG):
        raw, red = _edge_vector(co, o, c, n)
        vec[n] = (raw, co.fr_to_mont(red), co.dlog_expected(group, red, SEED_B, n))
        assert vec[n][2] != bytes(aff)

    def check(cx, got, n, windows, groups=1):
        assert _canon(co, group, got) == vec[n][2], (group, c, n, windows, groups)
        p = cx.profile()
        assert p["window_bits"] == c and p["num_windows"] == windows and p["window_groups"] == groups and p["n"] == n

    with pkg.Context([0]) as cx:
        cx.set_window_bits(c)
        cx.set_pipeline([1])
        for n in (N_SMALL, N_BIG):
            raw, mont, _ = vec[n]
            # 1. bases with the call (never folded), canonical (unreduced values among them) and Montgomery scalars
            check(cx, cx.msm(group, bases[:aff * n], raw, n, pkg.SCALAR_CANONICAL), n, w_plain)
            check(cx, cx.msm(group, bases[:aff * n], mont, n, pkg.SCALAR_MONTGOMERY), n, w_plain)
        # 2. resident bases that are not validated: no fold
        cx.set_bases(group, bases, N_BIG)
        d_raw = {}
        for n in (N_SMALL, N_BIG):
            check(cx, cx.msm(group, None, vec[n][0], n, pkg.SCALAR_CANONICAL), n, w_plain)
            # 3. scalars in device memory
            d_raw[n] = torch.frombuffer(bytearray(vec[n][0]), dtype=torch.uint8).cuda()
            torch.cuda.synchronize()
            check(cx, cx.msm_device(group, d_raw[n].data_ptr(), n, pkg.SCALAR_CANONICAL), n, w_plain)
        # 4. window groups: the sort of a later group runs beside the accumulate kernel of the one before, every group recodes from
        #    window 0 and keeps the digits of its own windows only
        for weights in ([1, 1], [1, 2, 1]):
            cx.set_pipeline(weights)
            check(cx, cx.msm(group, None, vec[N_BIG][0], N_BIG, pkg.SCALAR_CANONICAL), N_BIG, w_plain, len(weights))
            check(cx, cx.msm_device(group, d_raw[N_BIG].data_ptr(), N_BIG, pkg.SCALAR_CANONICAL), N_BIG, w_plain, len(weights))
            check(cx, cx.msm(group, None, vec[N_BIG][1], N_BIG, pkg.SCALAR_MONTGOMERY), N_BIG, w_plain, len(weights))
        cx.set_pipeline([1])
        # 5. validated set: s > (r - 1) / 2 becomes r - s with every sign inverted, one window fewer at c = 15 / 17
        assert cx.validate_bases(group) == 0
        for n in (N_SMALL, N_BIG):
            check(cx, cx.msm(group, None, vec[n][0], n, pkg.SCALAR_CANONICAL), n, w_fold)
            check(cx, cx.msm(group, None, vec[n][1], n, pkg.SCALAR_MONTGOMERY), n, w_fold)
            check(cx, cx.msm_device(group, d_raw[n].data_ptr(), n, pkg.SCALAR_CANONICAL), n, w_fold)
        cx.set_pipeline([1, 1])
        check(cx, cx.msm(group, None, vec[N_BIG][0], N_BIG, pkg.SCALAR_CANONICAL), N_BIG, w_fold, 2)
        cx.set_pipeline(None)
        # one point, one scalar: every digit of the result is that scalar's — with the fold (resident) and without (host base)
        base = bases[:aff]
        for s in _single_scalars(o, c):
            sb = du.scalar_bytes([s])
            want = _mul(o, group, base, s)
            assert _canon(co, group, cx.msm(group, base, sb, 1, pkg.SCALAR_CANONICAL)) == want, (group, c, hex(s), "host base")
            assert cx.profile()["num_windows"] == w_plain
            assert _canon(co, group, cx.msm(group, None, sb, 1, pkg.SCALAR_CANONICAL)) == want, (group, c, hex(s), "fold")
            assert cx.profile()["num_windows"] == w_fold
        cx.set_window_bits(0)
    # 6. precomputed tables: all windows share ONE bucket set (entry index = window * stride + i); a prefix call keeps the stride
    accepted = pkg.test_plan(N_BIG, c, group, True, N_BIG)["c"] == c
    with pkg.Context([0]) as cp:
        if not accepted:
            with pytest.raises(pkg.MsmError) as e:
                cp.set_bases_precomputed(group, bases, N_BIG, c)
            assert e.value.code == -1
            return
        cp.set_bases_precomputed(group, bases, N_BIG, c)
        for n in (N_BIG, N_SMALL):
            check(cp, cp.msm(group, None, vec[n][0], n, pkg.SCALAR_CANONICAL), n, w_plain)
            check(cp, cp.msm(group, None, vec[n][1], n, pkg.SCALAR_MONTGOMERY), n, w_plain)


# ------------------------------------------------------------------------------------------------ exceptional pairs
def _pool(co, o, group, count):
    F, aff = _curve(o, group)
    raw = co.gen_bases(group, SEED_B + 1, count, 4)
    return [o.affine_from_bytes(F, raw[aff * i:aff * (i + 1)]) for i in range(count)]


PATTERNS = ("PP", "P-PS", "QR(Q+R)", "PQR", "Px8", "P-P", "QR-(Q+R)", "P+m,-P-m", "PPP", "PP-P-P", "QR-(Q+R)SS", "SQ", "P-m,-P-m")


def _mixed_buckets(o, group, pool):
    """(bases, scalars) at c = 8: bucket m - 1 of window 0, m = 1 .. 128, holds the multiset of pattern m mod 13.  A point enters
    bucket m - 1 with sign + through the scalar m and with sign - through 256 - m (raw digit 256 - m > 128: digit -m, carry), so the
    negative entries also ALL land, with sign +, in bucket 0 of window 1 — a heavy bucket that mixes every pattern."""
    F, _ = _curve(o, group)
    neg = lambda p: o.aff_neg(F, p)
    pts, sc, kinds = [], [], set()
    for m in range(1, 129):
        P, Q, R, S = (pool[(m + k) % len(pool)] for k in (0, 5, 9, 14))
        QR = o.aff_add(F, Q, R)
        kind = PATTERNS[m % len(PATTERNS)]
        kinds.add(kind)
        plus, minus = {                                   # points entering with digit +m / with digit -m
            "PP": ([P, P], []), "PPP": ([P, P, P], []), "Px8": ([P] * 8, []),
            "P-P": ([P, neg(P)], []), "P-PS": ([P, neg(P), S], []), "PP-P-P": ([P, P, neg(P), neg(P)], []),
            "QR(Q+R)": ([Q, R, QR], []), "QR-(Q+R)": ([Q, R, neg(QR)], []), "QR-(Q+R)SS": ([Q, R, neg(QR), S, S], []),
            "P+m,-P-m": ([P], [neg(P)]),                  # the same point once the sign is applied: a doubling
            "P-m,-P-m": ([], [P, neg(P)]),                # a cancellation among negative digits
            "PQR": ([P, Q, R], []), "SQ": ([S, Q], []),
        }[kind]
        pts += plus + minus
        sc += [m] * len(plus) + [256 - m] * len(minus)
    assert kinds == set(PATTERNS)
    order = list(range(len(pts)))
    random.Random(8).shuffle(order)                       # neighbours in the vector belong to different buckets
    return [pts[i] for i in order], [sc[i] for i in order]


@pytest.mark.parametrize("group", GROUPS)
def test_a_wave_of_mixed_exceptional_buckets(pkg, co, o, group):
    """128 buckets of one window (two waves of k_accumulate, four of k_accumulate_g2_coop's lane pairs) whose lanes leave the hot loop
    at different entries — a doubling at the first, second or last addition, a cancellation, a sum that meets its own negative — next
    to lanes that never leave it.  The order of the entries inside a bucket is not deterministic (LDS atomics of the sort), so only
    the resulting point is asserted, against the oracle's double-and-add sum and its Pippenger on the same inputs."""
    F, aff = _curve(o, group)
    pts, sc = _mixed_buckets(o, group, _pool(co, o, group, 16))
    n = len(pts)
    assert 300 <= n <= 600
    bases = b"".join(o.affine_to_bytes(F, p) for p in pts)
    canon = du.scalar_bytes(sc)
    want = _canon(co, group, co.msm_naive(group, bases, canon, n))
    assert want == _canon(co, group, co.msm(group, bases, canon, n, 0, 4)) and want != bytes(aff)   # not vacuous
    with pkg.Context([0]) as cx:
        cx.set_window_bits(8)
        assert _canon(co, group, cx.msm(group, bases, canon, n, pkg.SCALAR_CANONICAL)) == want
        p = cx.profile()
        assert p["window_bits"] == 8 and p["num_windows"] == 32 and p["n"] == n
        assert _canon(co, group, cx.msm(group, bases, co.fr_to_mont(canon), n, pkg.SCALAR_MONTGOMERY)) == want
        cx.set_bases(group, bases, n)
        assert _canon(co, group, cx.msm(group, None, canon, n, pkg.SCALAR_CANONICAL)) == want
        cx.set_window_bits(0)
        assert _canon(co, group, cx.msm(group, None, canon, n, pkg.SCALAR_CANONICAL)) == want


@pytest.mark.parametrize("group", GROUPS)
def test_one_point_repeated(pkg, co, o, group):
    """3000 copies of one base with one scalar: every bucket that is not empty is heavy, every split item meets an exceptional pair
    at its FIRST addition (P + P) and the merge adds equal partial sums.  Closed form: (3000 s mod r) P.  With half of the bases
    negated everything cancels."""
    F, aff = _curve(o, group)
    n = 3000
    P = _pool(co, o, group, 16)[0]
    pb, nb = o.affine_to_bytes(F, P), o.affine_to_bytes(F, o.aff_neg(F, P))
    s = random.Random(0xB2).randrange(1, o.R_ORDER)
    sc = du.scalar_bytes([s] * n)
    want = _mul(o, group, pb, n * s)
    assert want != bytes(aff)
    with pkg.Context([0]) as cx:
        for c in (0, 12):
            cx.set_window_bits(c)
            assert _canon(co, group, cx.msm(group, pb * n, sc, n, pkg.SCALAR_CANONICAL)) == want, c
            p = cx.profile()
            assert p["max_items_per_bucket"] > 1 and (c == 0 or p["window_bits"] == c)
            assert _canon(co, group, cx.msm(group, (pb + nb) * (n // 2), sc, n, pkg.SCALAR_CANONICAL)) == bytes(aff), c
            assert cx.profile()["max_items_per_bucket"] > 1
            assert _canon(co, group, cx.msm(group, pb * (n // 2) + nb * (n // 2), sc, n, pkg.SCALAR_CANONICAL)) == bytes(aff), c
        cx.set_window_bits(0)


@pytest.mark.parametrize("group", GROUPS)
def test_bases_of_small_order(pkg, co, o, group):
    """About 200 bases from {T, -T, infinity} for points T of order 3, 11, 10177 (G1; (0, 2) among them) and 13, 23, 2713 (G2): nearly
    every addition of the MSM is a doubling, a cancellation or an addition to infinity.  Host bases: the integer s mod r multiplies
    the point, whatever its order (no sign fold).  Expected: sum ((s mod r) mod q) T with the big-int oracle."""
    from cofactor_util import SMALL_PRIMES, small_order_points

    F, aff = _curve(o, group)
    r = o.R_ORDER
    small = small_order_points(o, group)                                  # [T_q, -T_q] per prime q
    choices = [(small[2 * k + j], q) for k, q in enumerate(SMALL_PRIMES[group]) for j in (0, 1)]
    if group == "g1":
        assert o.on_curve(F, (0, 2)) and o.scalar_mul(F, (0, 2), 3) is o.INF
        choices += [((0, 2), 3), ((0, o.P - 2), 3)] * 2                   # weighted: a third of the bases have order 3
    choices += [(o.INF, 1)] * 2
    rnd = random.Random(0xB3)
    special = du.special_scalars(8, r)
    n = 208
    picks = [choices[rnd.randrange(len(choices))] for _ in range(n)]
    vals = [rnd.getrandbits(255) if i % 4 else special[(i // 4) % len(special)] for i in range(n)]
    assert any(v >= r for v in vals)
    want = o.INF
    for (T, q), v in zip(picks, vals):
        if T is not o.INF:
            want = o.aff_add(F, want, o.scalar_mul(F, T, (v % r) % q))
    want = o.affine_to_bytes(F, want) if want is not o.INF else bytes(aff)
    bases = b"".join(o.affine_to_bytes(F, T) if T is not o.INF else bytes(aff) for T, _ in picks)
    sc = du.scalar_bytes(vals)
    with pkg.Context([0]) as cx:
        for c in (8, 0):
            cx.set_window_bits(c)
            assert _canon(co, group, cx.msm(group, bases, sc, n, pkg.SCALAR_CANONICAL)) == want, c
            assert c == 0 or cx.profile()["window_bits"] == c
        cx.set_window_bits(0)
