"""Shared by tests/test_msm_reduce_cpu.py (CPU) and tests/test_gpu_msm_reduce.py (GPU): constructed bucket contents for the third stage of
the MSM (k_merge, k_reduce_coop, k_reduce_serial, k_combine: csrc/curve_kernels.cuh) and an integer model of those kernels' schedules.

Builder.  A scalar m 2^(c w) with 1 <= m <= 2^(c-1) has one non-zero digit: its base lands in bucket m of window w and nowhere else.  With
bases k G of the oracle's generator a test dictates every bucket as a known multiple of G, and every window sum is (sum m k mod r) G in
closed form, whatever the pipeline does.  A PATTERN is a mapping  bucket magnitude -> [k, ...]  for one window (k < 0 means r - k).

Model.  Points are discrete logarithms modulo r (None = infinity; every base lies in the subgroup of order r, so equal logarithms are equal
points).  The model restates the kernels' schedules step by step and lane by lane, with their ragged-lane rules and their wave-uniform
skips, and records for every addition that an occupied logical lane executes the STAGE and the OPERAND CLASS (generic, A = inf, B = inf,
both, A = B, A = -B): the complete addition is rendered four times across lanes (QuadG1, OctG2, PairG2, single lane), and a pattern set
only tests an exceptional case of it where the model says the case occurs.  Additions whose second operand is infinity by construction
(a lane beyond the window's buckets, a shuffle from beyond the wave, lane 0 of the comb step) are not recorded: the classes counted are
those of values."""
import os
import sys
from collections import namedtuple

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msm_digits_util as du  # noqa: E402

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001     # order of G1 / G2 (the CPU test holds it against the oracle's)
MERGE_FAN = 4
NLL_LOG = {"g1": 4, "g2": 5}         # logical lanes per wave of k_reduce_coop: QuadG1 / PairG2
COMBINE_LOG = {"g1": 4, "g2": 3}     # ... of k_combine and k_merge: QuadG1 / OctG2

GENERIC, A_INF, B_INF, BOTH_INF, EQUAL, OPPOSITE = "generic", "A=inf", "B=inf", "both inf", "A=B", "A=-B"
CLASSES = (GENERIC, A_INF, B_INF, BOTH_INF, EQUAL, OPPOSITE)
RUNNING, WEIGHTED, SCAN, CHAIN_DBL, CHAIN_ADD, COMB, BUTTERFLY, RIDER = ("running", "weighted", "scan", "chain-double", "chain-add", "comb",
                                                                         "butterfly", "rider")
COOP_STAGES = (RUNNING, WEIGHTED, SCAN, CHAIN_DBL, CHAIN_ADD, COMB, BUTTERFLY, RIDER)
SERIAL_STAGES = (RUNNING, WEIGHTED, CHAIN_DBL, CHAIN_ADD)
COMBINE_STAGES = (SCAN, COMB, BUTTERFLY, RIDER)
MERGE_STAGES = ("level 0", "level 1", "level 2")


# ------------------------------------------------------------------------------------------------ arithmetic on logarithms
def norm(k):
    """integer -> logarithm: None for a multiple of r"""
    return (k % R) or None


def classify(a, b):
    if a is None or b is None:
        return BOTH_INF if a is None and b is None else A_INF if a is None else B_INF
    return EQUAL if a == b else OPPOSITE if (a + b) % R == 0 else GENERIC


class Trace:
    """what the model's additions met: {stage: {class: count}}"""

    def __init__(self):
        self.seen = {}

    def add(self, stage, a, b, record=True):
        if record:
            st = self.seen.setdefault(stage, {})
            cl = classify(a, b)
            st[cl] = st.get(cl, 0) + 1
        if a is None or b is None:
            return b if a is None else a
        return norm(a + b)

    def merge(self, other):
        for stage, st in other.seen.items():
            mine = self.seen.setdefault(stage, {})
            for cl, k in st.items():
                mine[cl] = mine.get(cl, 0) + k

    def missing(self, stages, impossible):
        """(stage, class) pairs that never occurred and are not listed as impossible"""
        return [(s, cl) for s in stages for cl in CLASSES if (s, cl) not in impossible and not self.seen.get(s, {}).get(cl)]


# ------------------------------------------------------------------------------------------------ windows
Window = namedtuple("Window", "val occ")   # val: magnitude -> logarithm of the bucket (absent / None = infinity); occ: magnitudes with an entry


def window_of(pattern):
    return Window({m: norm(sum(ks)) for m, ks in pattern.items() if ks}, {m for m, ks in pattern.items() if ks})


def closed_form(pattern):
    """sum m k mod r, as an integer in [0, r)"""
    return sum(m * k for m, ks in pattern.items() for k in ks) % R


# ------------------------------------------------------------------------------------------------ k_reduce_coop
def _chain_bits(L):
    top = L.bit_length() - 1
    return [(L >> b) & 1 for b in range(top - 1, -1, -1)]


def _scan_comb_butterfly(log_ll, run, acc, live, trace, lp_of):
    """the closing steps k_reduce_coop and k_combine share: suffix scan of `run`, acc += (lane 0 ? inf : lp_of(run)), butterfly over the
    lanes with the rider.  live[l]: logical lane l holds values (not padding).  Returns (rider's value, lane 0's acc)."""
    nll = 1 << log_ll
    for s in range(log_ll):
        d = 1 << s
        run = [trace.add(SCAN, run[l], run[l + d], live[l] and live[l + d]) if l + d < nll else run[l] for l in range(nll)]
    lp = lp_of(run)
    acc = [acc[0]] + [trace.add(COMB, acc[l], lp[l], live[l]) for l in range(1, nll)]
    ride = lp[0]
    for k in range(log_ll):
        d = (nll // 2) >> k
        acc = [trace.add(BUTTERFLY, acc[l], acc[l + d], live[l] and live[l + d]) if l < d else acc[l] for l in range(nll)]
        ride = trace.add(RIDER, ride, ride)
    return ride, acc[0]


def reduce_coop(log_ll, L, nb, win, trace):
    """k_reduce_coop<CS> on one window: one wave per chunk of K = NLL L buckets -> [(K S, T)] per chunk"""
    nll = 1 << log_ll
    K = nll * L
    cpw = -(-nb // K)
    bits = _chain_bits(L)
    pairs = []
    for j in range(cpw):
        first = [(j * nll + l) * L for l in range(nll)]
        cnt = [0 if f >= nb else min(L, nb - f) for f in first]
        live = [c > 0 for c in cnt]
        full = lambda l, rel: rel < cnt[l] and (first[l] + rel + 1) in win.occ
        if not any(full(l, rel) for l in range(nll) for rel in range(L)):
            pairs.append((None, None))                                   # the wave leaves early
            continue
        run, acc, fr = [None] * nll, [None] * nll, [False] * nll
        for p in range(L):
            rel = L - 1 - p
            fB = [full(l, rel) for l in range(nll)]
            fr = [a or b for a, b in zip(fr, fB)]
            if any(fB):                                                  # run += B_rel, skipped when no lane's bucket holds an entry
                run = [trace.add(RUNNING, run[l], win.val.get(first[l] + rel + 1)) if rel < cnt[l] else run[l] for l in range(nll)]
            if any(fr):                                                  # acc += run, skipped while every lane's run is still infinity
                acc = [trace.add(WEIGHTED, acc[l], run[l], rel < cnt[l]) for l in range(nll)]

        def lp_of(run):
            lp = list(run)
            for bit in bits:
                lp = [trace.add(CHAIN_DBL, x, x, live[l]) for l, x in enumerate(lp)]
                if bit:
                    lp = [trace.add(CHAIN_ADD, x, run[l], live[l]) for l, x in enumerate(lp)]
            return lp

        ride, t = _scan_comb_butterfly(log_ll, run, acc, live, trace, lp_of)
        S = norm(sum(win.val.get(m) or 0 for m in range(j * K + 1, min(nb, j * K + K) + 1)))
        T = norm(sum((m - j * K) * (win.val.get(m) or 0) for m in range(j * K + 1, min(nb, j * K + K) + 1)))
        assert ride == norm(K * (S or 0)) and t == T, ("k_reduce_coop model", log_ll, L, nb, j)
        pairs.append((ride, t))
    return pairs


# ------------------------------------------------------------------------------------------------ k_reduce_serial
def reduce_serial(L, nb, wins, trace):
    """k_reduce_serial on ALL bucket windows of a call (a wave's 64 lanes may span windows, the skips are wave-uniform): lane g = (w, j)
    covers L buckets -> per window [(L S, T)] per lane.  The idle lanes of the last wave repeat the last lane, so they never change a ballot."""
    lpw = -(-nb // L)
    nlanes = lpw * len(wins)
    bits = _chain_bits(L)
    out = [[None] * lpw for _ in wins]
    for wave in range(0, nlanes, 64):
        lanes = list(range(wave, min(nlanes, wave + 64)))
        geo = []
        for g in lanes:
            w, j = divmod(g, lpw)
            geo.append((wins[w], j * L, min(L, nb - j * L)))
        full = lambda i, rel: rel < geo[i][2] and (geo[i][1] + rel + 1) in geo[i][0].occ
        n = len(lanes)
        if not any(full(i, rel) for i in range(n) for rel in range(L)):
            for g in lanes:
                out[g // lpw][g % lpw] = (None, None)
            continue
        run, acc, fr = [None] * n, [None] * n, [False] * n
        for p in range(L):
            rel = L - 1 - p
            fB = [full(i, rel) for i in range(n)]
            fr = [a or b for a, b in zip(fr, fB)]
            if any(fB):
                run = [trace.add(RUNNING, run[i], geo[i][0].val.get(geo[i][1] + rel + 1)) if rel < geo[i][2] else run[i] for i in range(n)]
            if any(fr):
                acc = [trace.add(WEIGHTED, acc[i], run[i], rel < geo[i][2]) for i in range(n)]
        S = list(run)
        for bit in bits:
            run = [trace.add(CHAIN_DBL, x, x) for x in run]
            if bit:
                run = [trace.add(CHAIN_ADD, x, S[i]) for i, x in enumerate(run)]
        for i, g in enumerate(lanes):
            win, f, c = geo[i]
            assert run[i] == norm(L * sum(win.val.get(m) or 0 for m in range(f + 1, f + c + 1))), ("k_reduce_serial model", L, nb, g)
            assert acc[i] == norm(sum((m - f) * (win.val.get(m) or 0) for m in range(f + 1, f + c + 1))), ("k_reduce_serial model", L, nb, g)
            out[g // lpw][g % lpw] = (run[i], acc[i])
    return out


# ------------------------------------------------------------------------------------------------ k_combine
def combine(log_ll, pairs, trace):
    """every level of k_combine<CS> over one window's pairs (S'_j, T_j) -> (the window sum, number of levels, [pairs per level going in])"""
    nll = 1 << log_ll
    levels, sizes = 0, []
    while True:
        cpw_in = len(pairs)
        cpw_out = -(-cpw_in // nll)
        sizes.append(cpw_in)
        levels += 1
        nxt = []
        for g in range(cpw_out):
            live = [g * nll + l < cpw_in for l in range(nll)]
            run = [pairs[g * nll + l][0] if live[l] else None for l in range(nll)]
            acc = [pairs[g * nll + l][1] if live[l] else None for l in range(nll)]
            if cpw_in > 1:
                nxt.append(_scan_comb_butterfly(log_ll, run, acc, live, trace, lambda r: r))
            else:
                nxt.append((None, acc[0]))                               # one pair: T is the window sum as it stands
        if cpw_out == 1:
            return nxt[0][1], levels, sizes
        pairs = nxt


def window_sum_coop(group, L, nb, win, t_reduce, t_combine):
    total, levels, sizes = combine(COMBINE_LOG[group], reduce_coop(NLL_LOG[group], L, nb, win, t_reduce), t_combine)
    return total, levels, sizes


# ------------------------------------------------------------------------------------------------ k_merge
def merge(items, trace):
    """k_merge's fan-in tree over the item sums of ONE split bucket (levels d = 1, 4, 16, ..; level 0 lists every 4th item, every level
    hands the items that accumulate again to the next one) -> the bucket"""
    it = list(items)
    n, d, level = len(it), 1, 0
    lst = list(range(0, n, MERGE_FAN))
    while d < n:
        nxt = []
        for k in lst:
            room = (n - 1 - k) // d if n - 1 - k >= d else 0
            for t in range(1, min(room, MERGE_FAN - 1) + 1):
                it[k] = trace.add("level %d" % level, it[k], it[k + t * d])
            if k % (MERGE_FAN * MERGE_FAN * d) == 0 and k + MERGE_FAN * d < n:
                nxt.append(k)
        lst, d, level = nxt, d * MERGE_FAN, level + 1
    return it[0]


def items_of(entries, logT):
    """the schedule's rule (sort_kernels.cuh items_of): a bucket beyond T = 2^logT entries is cut into items of S = max(16, T / 4)"""
    S = 1 << max(4, logT - 2)
    return [entries[i:i + S] for i in range(0, len(entries), S)] if len(entries) > (1 << logT) else [entries]


def merge_counts(logT):
    """item counts of the split bucket: 2, 4, 5, 16, 17 as far as they can occur.  A bucket is split only beyond T entries, into items of
    S = max(16, T / 4): at least T / S + 1 items (3 at logT = 5, 5 from logT = 6 on), so 2 never occurs (nor 4 from logT = 6 on) and the
    smallest count that does takes its place."""
    least = (1 << logT >> max(4, logT - 2)) + 1
    return tuple(sorted({least} | {k for k in (2, 4, 5, 16, 17) if k >= least}))


MERGE_KINDS = ("all P", "alternating", "cancelled by the last", "head cancels", "tail cancels", "tail equals head")


def merge_entries(kind, count, logT):
    """the logarithms of one split bucket of `count` items (the last one of one or two entries, so the counts sit at the item boundaries).
    Which entries share an item follows the order of the entries; the model takes them in the order given."""
    S = 1 << max(4, logT - 2)
    n = (count - 1) * S + 1
    assert n > (1 << logT) and len(items_of([0] * (n + 1), logT)) == count, (count, logT)
    if kind == "all P":                        # equal item sums: the merge doubles
        return [1] * n
    if kind == "alternating":                  # every item sums to infinity (the last one holds two entries)
        return [1 if i % 2 == 0 else -1 for i in range(n - 1)] + [1, -1]
    if kind == "cancelled by the last":        # the merged bucket is infinity, at the tree's last addition
        return [1] * (n - 1) + [-(n - 1)]
    if kind == "head cancels":                 # A = infinity meets a finite last item
        return [1 if i % 2 == 0 else -1 for i in range(n - 1)] + [7]
    if kind == "tail cancels":                 # finite sums meet items that are infinity
        return [1] * S + [1 if i % 2 == 0 else -1 for i in range(n - 1 - S)] + [5, -5]
    if kind == "tail equals head":             # the last item equals the sum of all before it
        return [1] * (n - 1) + [n - 1]
    raise KeyError(kind)


# ------------------------------------------------------------------------------------------------ patterns
Geo = namedtuple("Geo", "nb L nll K cpw")


def geo_coop(group, c, L):
    nb, nll = 1 << (c - 1), 1 << NLL_LOG[group]
    return Geo(nb, L, nll, nll * L, -(-nb // (nll * L)))


def geo_serial(c, L):
    nb = 1 << (c - 1)
    return Geo(nb, L, 1, L, -(-nb // L))


def _clip(g, pat):
    return {m: ks for m, ks in pat.items() if 1 <= m <= g.nb and ks}


def _rnd(seed):
    import random

    return random.Random(seed)


def patterns(g):
    """[(name, pattern)] for the geometry g: the named cases of the third stage.  Every pattern is also a valid input of every other
    geometry with the same nb (only what it aims at moves)."""
    nb, L, K = g.nb, g.L, g.K
    last0 = (g.cpw - 1) * K                       # buckets before the last chunk (ragged when nb is no multiple of K)
    last_lane = ((nb - 1) // L) * L + 1           # first bucket of the last occupied lane
    out = []
    singles = []
    for m in (1, 2, L, L + 1, K, K + 1, nb, last0, last0 + 1, last_lane):
        if 1 <= m <= nb and m not in singles:
            singles.append(m)
    for m in singles:
        out.append(("single %d" % m, {m: [1]}))
    # every bucket holds G: every lane doubles in the same step (beyond 1024 buckets: the first chunk, the last one and every K-th bucket)
    dense = range(1, nb + 1) if nb <= 1024 else sorted(set(range(1, K + 1)) | set(range(last0 + 1, nb + 1)) | set(range(K, nb + 1, K)))
    out.append(("every bucket G", {m: [1] for m in dense}))
    # every chunk holds the same content: the suffix scans of the combine add equal values
    same = {}
    for j in range(g.cpw):
        for rel, k in ((0, 1), (min(L, K - 1), 2), (K - 1, 3)):
            same.setdefault(j * K + rel + 1, []).append(k)
    out.append(("every chunk the same", _clip(g, same)))
    t = max(L, 3)
    out.append(("P, -P adjacent", _clip(g, {t: [3], t - 1: [-3], t - 2: [5]})))                 # the running sum passes through infinity
    out.append(("P on top, -2P below", _clip(g, {t: [1], t - 1: [-2], t - 2: [4]})))            # the weighted sum passes through infinity
    out.append(("lane sums cancel", _clip(g, {L + 1: [3], 2 * L + 1: [-3], 1: [2]})))           # the scan cancels
    out.append(("S inf, T finite", {1: [1], 2: [-1]}))                                          # the rider doubles infinity beside a finite T
    out.append(("T inf, S finite", {1: [-2], 2: [1]}))
    a = K if 2 * K <= nb else 1
    out.append(("window sums to infinity", {2 * a: [1], a: [-2]}))                              # store_jac_raw's zero path
    j = 1 if g.cpw > 1 else 0
    out.append(("one chunk only", _clip(g, {j * K + 1: [1], j * K + min(K, 3 * L + 2): [2], j * K + K: [-1]})))
    out.append(("one lane only", _clip(g, {(2 % g.nll) * L + rel + 1: [rel + 1] for rel in range(L)})))
    out.append(("ragged tail only", _clip(g, {last0 + 1: [1], (last0 + 1 + nb) // 2: [2], nb: [3], nb - 1: [-3]})))
    out.append(("empty", {}))
    # lanes and chunks whose partial sums meet each other again: small multiples of G at the lane and chunk boundaries, so that equal and
    # opposite operands occur in the scan, the comb step and the butterfly of both kernels
    for seed in range(6):
        rnd, pat = _rnd(1000 + seed), {}
        where = [1, 2, L, L + 1, 2 * L, 2 * L + 1, K, K + 1, 2 * K, 2 * K + 1, last0 + 1, nb] + [rnd.randrange(1, nb + 1) for _ in range(4)]
        for m in where:
            if 1 <= m <= nb and rnd.random() < 0.7:
                pat.setdefault(m, []).append(rnd.choice((1, -1, 2, -2, 3, -3)))
        out.append(("small multiples %d" % seed, pat))
    out += _aimed(g)
    return [(name, pat) for name, pat in out if pat or name == "empty"]


def _aimed(g):
    """patterns solved for one operand class of one stage each (bucket rel of lane l of chunk j is magnitude j K + l L + rel + 1)"""
    nb, L, K, nll = g.nb, g.L, g.K, g.nll
    out = []
    at = lambda j, l, rel=0: j * K + l * L + rel + 1
    if nll >= 4 and K <= nb:
        # comb step, lane 1: T_1 = x (bucket rel 0), L P_1 = L x' with the lanes above; A = B needs T_1 = L P_1, A = -B the negative
        out.append(("comb equal", _clip(g, {at(0, 1, L - 1): [1]})))                              # T_1 = L G = L P_1
        out.append(("comb opposite", _clip(g, {at(0, 1, L - 1): [1], at(0, 2): [-2]})))           # T_1 = L G, P_1 = -G
        out.append(("comb A inf", _clip(g, {at(0, 2): [1]})))                                     # T_1 = inf, P_1 = G
        out.append(("comb B inf", _clip(g, {at(0, 1): [1], at(0, 2): [-1]})))                     # T_1 = G, P_1 = inf
        # butterfly, first step (lanes l and l + NLL/2): the lanes enter it with V_0 = T_0 and V_l = T_l + L P_l
        h = nll // 2
        # lane h holds y at rel 0: T_h = y, P_h = y: V_h = (1 + L) y;  P_l = y for every l <= h, so V_l = L y for 1 <= l < h, V_0 = T_0
        out.append(("butterfly lane 0", _clip(g, {at(0, h): [1], at(0, 0): [1 + L]})))            # V_0 = (1 + L) G = V_h: A = B
        out.append(("butterfly lane 0 opposite", _clip(g, {at(0, h): [1], at(0, 0): [-(1 + L)]})))
    if g.cpw >= 2:
        # combine: pairs (K S_j, T_j) of chunks 0 and 1
        out.append(("combine scan equal", _clip(g, {at(0, 0): [1], at(1, 0): [1]})))              # S'_0 = S'_1
        out.append(("combine scan opposite", _clip(g, {at(0, 0): [1], at(1, 0): [-1]})))
        out.append(("combine comb equal", _clip(g, {2 * K: [1]})))                                # T_1 = K G = S'_1
        out.append(("combine comb opposite", _clip(g, {K + 1: [-2 * K], 2 * K: [1 + K]})))        # T_1 = (K^2 - K) G = -S'_1
        out.append(("combine comb A inf", _clip(g, {K + 1: [-2], K + 2: [1]})))                   # T_1 = inf, S_1 = -G
        out.append(("combine comb B inf", _clip(g, {K + 1: [1], K + 2: [-1]})))                   # S_1 = inf, T_1 = -G
        out.append(("combine butterfly equal", _clip(g, {1: [2 * K], 2 * K: [1]})))               # V_0 = T_0 = 2K G, V_1 = T_1 + S'_1 = K G + K G
        out.append(("combine butterfly opposite", _clip(g, {1: [-2 * K], 2 * K: [1]})))
    return out


def max_magnitude(c, w, fold=False):
    """largest bucket of window w a scalar below r (below (r + 1) / 2 with the fold, so that it IS folded) can reach with one digit"""
    lim = ((R + 1) // 2 - 1) if fold else R - 1
    return min(1 << (c - 1), lim >> (c * w))


def place(named, c, fold=False):
    """spread [(name, pattern)] over the windows of as many calls as it takes, in order; the short top windows get the first pattern that
    fits them -> [[(window, name, pattern)] per call]"""
    W = du.windows(c, fold)
    caps = [max_magnitude(c, w, fold) for w in range(W)]
    rest, calls = list(named), []
    while rest:
        call = []
        for w in range(W):
            pick = next((i for i, (_, p) in enumerate(rest) if max(p, default=0) <= caps[w]), None)
            if pick is not None and caps[w] >= 1:
                call.append((w,) + rest.pop(pick))
        assert call, "a pattern fits no window"
        calls.append(call)
    return calls


# ------------------------------------------------------------------------------------------------ builder
Built = namedtuple("Built", "bases scalars n expected total logs")

_GEN = {}


def mul_gen(co, group, k):
    key = (group, k % R)
    if key not in _GEN:
        _GEN[key] = co.mul_gen(group, k % R)
    return _GEN[key]


def build(co, group, c, placed, fold=False):
    """placed: [(window, pattern)] (or (window, name, pattern)).  Returns the bases k G (None with co=None), the canonical scalars, n, the
    expected logarithm per window (sum m k mod r, 0 = infinity) and of the whole MSM, and the bases' logarithms.  With fold (a validated
    resident set) the scalar is r - m 2^(c w) > (r - 1) / 2 and the base -k G: the library recodes m 2^(c w) with every sign inverted, so
    the entry lands in the same bucket with a negative sign and the bucket holds k G all the same."""
    W = du.windows(c, fold)
    logs, vals, expected = [], [], [0] * W
    for item in placed:
        w, pat = item[0], item[-1]
        assert 0 <= w < W
        for m in sorted(pat):
            assert 1 <= m <= max_magnitude(c, w, fold), (c, w, m)
            for k in pat[m]:
                s = m << (c * w)
                if fold:
                    s, k = R - s, -k
                d, _ = du.recode(s, c, fold, R)
                assert [i for i, x in enumerate(d) if x] == [w] and d[w] == (-m if fold else m), (c, w, m, d)
                logs.append(k % R)
                vals.append(s)
                expected[w] = (expected[w] + m * (-k if fold else k)) % R
    total = sum(s * k for s, k in zip(vals, logs)) % R
    assert total == sum(e << (c * w) for w, e in enumerate(expected)) % R
    bases = b"".join(mul_gen(co, group, k) for k in logs) if co is not None else None
    return Built(bases, du.scalar_bytes(vals), len(vals), expected, total, logs)


# ------------------------------------------------------------------------------------------------ the geometries of the GPU test
def _smallest_c(nll, L):
    c = 7
    while (1 << (c - 1)) < 2 * nll * L:
        c += 1
    return c


COOP_L = {"g1": (1, 2, 3, 5, 7, 8, 15, 16, 33, 64), "g2": (1, 2, 3, 7, 8, 21, 64)}
# (L, c): at least two chunks per window at the smallest c; then ONE chunk exactly (nb = NLL L: the cpw_in == 1 path of k_combine); then
# many chunks: G1 512 per window (three combine levels: 512 -> 32 -> 2 -> 1), G2 64 (two OctG2 levels, 64 -> 8 -> 1, both exact) and 32
# (32 -> 4 -> 1: the second level's 4 pairs do not fill its 8 lanes)
COOP_CASES = {
    "g1": [(L, _smallest_c(16, L)) for L in COOP_L["g1"]] + [(4, 7), (1, 14)],
    "g2": [(L, _smallest_c(32, L)) for L in COOP_L["g2"]] + [(2, 7), (1, 12), (1, 11)],
}
SERIAL_CASES = [(L, c) for c in (7, 10) for L in (1, 2, 3, 8, 53, 64)]
