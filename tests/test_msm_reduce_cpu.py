"""CPU half of the constructed-bucket tests of the MSM's third stage (tests/msm_reduce_util.py; the GPU half is
tests/test_gpu_msm_reduce.py): the integer model of k_reduce_coop / k_reduce_serial / k_combine / k_merge reproduces the closed form
sum m k for every geometry the GPU test forces, the built vectors mean what they claim under the C oracle's Pippenger, and — the
coverage condition — the pattern set makes every operand class of the complete addition occur in every stage of every kernel and lane
scheme where it can occur at all.  The condition is a property of the INPUTS, proven here; it is not a measurement of the kernels."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msm_digits_util as du  # noqa: E402
import msm_reduce_util as ru  # noqa: E402

_T = {}


def _coop_traces(group):
    """model of every forced geometry of the group over its patterns -> (trace of k_reduce_coop, trace of k_combine, facts)"""
    if group in _T:
        return _T[group]
    t_red, t_comb, facts = ru.Trace(), ru.Trace(), []
    for L, c in ru.COOP_CASES[group]:
        g = ru.geo_coop(group, c, L)
        # the CPU test recomputes the geometry itself
        nll = 16 if group == "g1" else 32
        assert g.nll == nll and g.K == nll * L and g.nb == 1 << (c - 1) and g.cpw == -(-g.nb // (nll * L)) and 1 <= L <= min(64, g.nb // nll)
        for name, pat in ru.patterns(g):
            total, levels, sizes = ru.window_sum_coop(group, L, g.nb, ru.window_of(pat), t_red, t_comb)
            assert (total or 0) == ru.closed_form(pat), (group, L, c, name)
        facts.append((L, c, g.cpw, levels, sizes))
    _T[group] = (t_red, t_comb, facts)
    return _T[group]


def _serial_traces():
    if "serial" in _T:
        return _T["serial"]
    t_red, t_comb, facts = ru.Trace(), ru.Trace(), []
    for L, c in ru.SERIAL_CASES:
        g = ru.geo_serial(c, L)
        assert g.nb == 1 << (c - 1) and g.cpw == -(-g.nb // L)
        W = du.windows(c, False)
        for call in ru.place(ru.patterns(g), c):
            pats = [{} for _ in range(W)]
            for w, name, pat in call:
                pats[w] = pat
            pairs = ru.reduce_serial(L, g.nb, [ru.window_of(p) for p in pats], t_red)
            for w in range(W):
                total, levels, sizes = ru.combine(4, pairs[w], t_comb)
                assert (total or 0) == ru.closed_form(pats[w]), (L, c, w)
        facts.append((L, c, g.cpw, g.cpw * W))
    _T["serial"] = (t_red, t_comb, facts)
    return _T["serial"]


def test_group_order(o):
    assert ru.R == o.R_ORDER


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_model_equals_closed_form_coop(group):
    """k_reduce_coop + every k_combine level, per window, at every (L, c) of the GPU test (the model also asserts every chunk's pair
    (K S, T) against its definition)"""
    _, _, facts = _coop_traces(group)
    by = {(L, c): (cpw, levels, sizes) for L, c, cpw, levels, sizes in facts}
    for L in ru.COOP_L[group]:
        c = next(c for (l, c) in by if l == L and by[l, c][0] >= 2)
        assert by[L, c][0] >= 2 and (c == 7 or (1 << (c - 2)) < 2 * (16 if group == "g1" else 32) * L)    # the smallest c with two chunks
    if group == "g1":
        assert by[4, 7] == (1, 1, [1])                       # one chunk: the cpw_in == 1 path
        assert by[1, 14] == (512, 3, [512, 32, 2])           # three levels, the last one's input does not fill the 16 lanes
    else:
        assert by[2, 7] == (1, 1, [1])
        assert by[1, 12] == (64, 2, [64, 8])                 # two OctG2 levels, both exact
        assert by[1, 11] == (32, 2, [32, 4])                 # ... and one whose second level has 4 pairs on 8 lanes
    assert any(nb_ragged for nb_ragged in ((1 << (c - 1)) % (L * (16 if group == "g1" else 32)) for L, c in by))   # ragged last chunks exist


def test_model_equals_closed_form_serial():
    _, _, facts = _serial_traces()
    by = {(L, c): (lpw, lanes) for L, c, lpw, lanes in facts}
    assert by[53, 7] == (2, 74) and 74 % 64 != 0             # two lanes per window, the second of 11 buckets; idle lanes in the last wave
    assert by[64, 7] == (1, 37) and by[1, 10] == (512, 512 * 26)


def test_model_equals_closed_form_shared_bucket_set():
    """precomputed tables: every window's entries meet in ONE bucket set, a base of window w counts 2^(c w) times"""
    c = 8
    g = ru.geo_coop("g1", c, 4)
    placed = ru.place(ru.patterns(g), c)[0]
    b = ru.build(None, "g1", c, placed)
    val = {}
    for w, _, pat in placed:
        for m, ks in pat.items():
            val.setdefault(m, []).extend(k << (c * w) for k in ks)
    total, _, _ = ru.window_sum_coop("g1", 4, g.nb, ru.window_of(val), ru.Trace(), ru.Trace())
    assert (total or 0) == b.total


def test_model_merge():
    for logT in (5, 6, 8):
        for count in ru.merge_counts(logT):
            for kind in ru.MERGE_KINDS:
                e = ru.merge_entries(kind, count, logT)
                items = ru.items_of(e, logT)
                assert len(items) == count
                got = ru.merge([ru.norm(sum(i)) for i in items], ru.Trace())
                assert got == ru.norm(sum(e)), (kind, count, logT)
    assert ru.merge([1, 2, 3, 4, 5], ru.Trace()) == 15 and ru.merge([None, None], ru.Trace()) is None


@pytest.mark.parametrize("group,c,L,fold", [("g1", 7, 2, False), ("g2", 8, 2, False), ("g1", 8, 3, True)])
def test_built_vectors_under_the_oracle(co, group, c, L, fold):
    """the C oracle's Pippenger over the built bases and scalars gives (total) G: the vectors mean what the builder says"""
    g = ru.geo_coop(group, c, L)
    for call in ru.place(ru.patterns(g), c, fold)[:2]:
        b = ru.build(co, group, c, call, fold)
        assert b.n >= 1 and any(b.expected)
        if fold:
            assert all(int.from_bytes(b.scalars[32 * i:32 * i + 32], "little") > (ru.R - 1) // 2 for i in range(b.n))
        assert co.to_affine(group, co.msm(group, b.bases, b.scalars, b.n, 0, 4)) == co.mul_gen(group, b.total)


# (stage, class) pairs that cannot occur, with the reason
_DOUBLING = "the step adds a value to itself"
_MULTIPLE = "A = m R with 2 <= m < L <= 64 and B = R: both are infinity or neither, and m R = +-R needs (m -+ 1) R = inf, R of prime order r"
IMPOSSIBLE_REDUCE = {
    (ru.CHAIN_DBL, ru.GENERIC): _DOUBLING, (ru.CHAIN_DBL, ru.A_INF): _DOUBLING, (ru.CHAIN_DBL, ru.B_INF): _DOUBLING,
    (ru.CHAIN_DBL, ru.OPPOSITE): _DOUBLING + " (and no point has order 2)",
    (ru.CHAIN_ADD, ru.A_INF): _MULTIPLE, (ru.CHAIN_ADD, ru.B_INF): _MULTIPLE, (ru.CHAIN_ADD, ru.EQUAL): _MULTIPLE, (ru.CHAIN_ADD, ru.OPPOSITE): _MULTIPLE,
    (ru.RIDER, ru.GENERIC): _DOUBLING, (ru.RIDER, ru.A_INF): _DOUBLING, (ru.RIDER, ru.B_INF): _DOUBLING,
    (ru.RIDER, ru.OPPOSITE): _DOUBLING + " (and no point has order 2)",
}
IMPOSSIBLE_COMBINE = {k: v for k, v in IMPOSSIBLE_REDUCE.items() if k[0] == ru.RIDER}
IMPOSSIBLE_MERGE = {}


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_coverage_condition_coop(group):
    """k_reduce_coop at LOG_LL 4 (QuadG1) / 5 (PairG2) and k_combine at LOG_LL 4 (QuadG1) / 3 (OctG2)"""
    t_red, t_comb, _ = _coop_traces(group)
    assert t_red.missing(ru.COOP_STAGES, IMPOSSIBLE_REDUCE) == [], t_red.seen
    assert t_comb.missing(ru.COMBINE_STAGES, IMPOSSIBLE_COMBINE) == [], t_comb.seen
    for stage, cl in IMPOSSIBLE_REDUCE:
        assert not t_red.seen.get(stage, {}).get(cl) and not t_comb.seen.get(stage, {}).get(cl), (stage, cl)   # the list is no wider than it must be


def test_coverage_condition_serial():
    t_red, t_comb, _ = _serial_traces()
    assert t_red.missing(ru.SERIAL_STAGES, IMPOSSIBLE_REDUCE) == [], t_red.seen
    assert t_comb.missing(ru.COMBINE_STAGES, IMPOSSIBLE_COMBINE) == [], t_comb.seen


def test_coverage_condition_merge():
    """over the split buckets of the GPU test, in the order the builder emits their entries (the sort's LDS atomics may order a bucket's
    entries differently on the device: what is asserted there is the merged bucket, which no order changes)"""
    t = ru.Trace()
    assert ru.merge_counts(5) == (3, 4, 5, 16, 17) and ru.merge_counts(6) == ru.merge_counts(9) == (5, 16, 17)
    for count in ru.merge_counts(5):
        for kind in ru.MERGE_KINDS:
            ru.merge([ru.norm(sum(i)) for i in ru.items_of(ru.merge_entries(kind, count, 5), 5)], t)
    assert t.missing(ru.MERGE_STAGES, IMPOSSIBLE_MERGE) == [], t.seen
