"""Raw-limb operands at the edges of the device field arithmetic's documented contracts, and the checker of the results.

Shared by tests/test_field_edges_cpu.py (host build of csrc/fp28.cuh + ec.cuh) and tests/test_gpu_field_edges.py (the device, through
mi_test_field_op).  The op table itself lives in csrc/field_test_ops.cuh; this file knows, per op name,
  * the INPUT contract, every number of which is quoted from the comment of the function under test, asserted on every vector before it
    is used (`legal`): a failing vector is then never a test-design error;
  * the vectors (`gen`): deterministic from SEED, a few hundred per op, in classes (tag prefix): maxcol (13 low limbs at the limb bound,
    limb 13 the largest under the value bound), neg (most negative signed Karatsuba columns), value (0, 1, p-1, p, p+1, 2p-1, the top of a
    K p contract, both representations of zero), spell (non-exact spellings: a limb of 2^28 borrowed from the next one), slow (exact values
    with l[0] == 0 or l[0] == P[0] that are neither 0 nor p), pattern (alternating / single-hot limbs), random (seeded N-form values over
    the full legal range), exc (xyzz_madd: exceptional pairs; line_add: T = +-Q), zero (line steps: a coordinate of T, xP or yP zero in
    every spelling), inf (line steps: the same vector with the sink's infinity flag);
  * the REFERENCE (`ref`): the mathematical value with Python integers — value = sum l[k] 2^(28k); a multiplier returns a number
    = (sum of products) 2^-392 (mod p); linear ops return a +- b + K p as an exact integer; Fp2 uses u^2 = -1; xyzz_madd its polynomial
    formulas — and the OUTPUT contract the comment promises (value range, limb form).
`model_peak` restates the column arithmetic only to REPORT how close to the 64-bit limit a vector drives a column; no verdict uses it.
"""
import os
import random
import re
from math import isqrt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0xF1E1D

P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
W, NL = 28, 14
MASK = (1 << W) - 1
R = 1 << (W * NL)                 # Montgomery radix 2^392
RINV = pow(R, -1, P)
RP = R * P                        # "a*b < 2^392 p"
E_MAX = MASK                      # exact limbs: < 2^28
N_MAX = (1 << 28) + 15            # fp28.cuh: "N-form: limbs l[0..12] <= 2^28 + 15"
MUL_LAZY_MAX = isqrt(1 << 59) - 1 # fp_mul: "limbs < 2^29.5 are still safe"
SPREAD_LO = (1 << 28) + 64        # fp_sub_lazy: "b must have limbs <= SPREAD_LO"
SUB_LAZY_GROW = (1 << 29) + 68    # fp_sub_lazy: "result limbs < a + 2^29 + 68"
WIDE_MAX = 3 * (1 << 28) - 1      # fp_sub8_lazy_wide: "b is a lazy sum of up to three exact values (limbs < 3 * 2^28)"
COL_LAZY = (1 << 64) - (1 << 60)  # fp_add_lazy: "a multiplication takes operands with 14 * la * lb < 2^64 - 2^60"
LOWSUM = sum(1 << (W * k) for k in range(NL - 1))


def _consts():
    text = open(os.path.join(ROOT, "ark-blst_amd", "csrc", "fp28_consts.h")).read()
    tab = {}
    for name, body in re.findall(r"uint32_t (\w+)\[14\] = \{([^}]*)\}", text):
        tab[name] = [int(x.strip().rstrip("u"), 16) for x in body.split(",")]
    tab["PINV"] = int(re.search(r"PINV = (0x[0-9a-f]+)u", text).group(1), 16)
    return tab


C = _consts()


def val(l):
    return sum(int(x) << (W * k) for k, x in enumerate(l))


def exact(v):
    """exact limbs: l[0..12] < 2^28, the rest in l[13]"""
    assert 0 <= v < 1 << (W * (NL - 1) + 32)
    return [(v >> (W * k)) & MASK for k in range(NL - 1)] + [v >> (W * (NL - 1))]


def maxlow(vbound, low=N_MAX):
    """13 low limbs at `low`, limb 13 the largest that keeps the value below vbound"""
    base = low * LOWSUM
    assert vbound > base
    return [low] * (NL - 1) + [(vbound - 1 - base) >> (W * (NL - 1))]


def borrow(l, k):
    """the same value with 2^28 of limb k borrowed from limb k + 1 (None when limb k + 1 is zero)"""
    if k >= NL - 1 or l[k + 1] == 0:
        return None
    r = list(l)
    r[k] += 1 << W
    r[k + 1] -= 1
    return r


def rand_nform(rnd, vbound, low=N_MAX):
    while True:
        l = [rnd.randrange(low + 1) for _ in range(NL - 1)] + [rnd.randrange(((vbound - 1) >> (W * (NL - 1))) + 1)]
        if val(l) < vbound:
            return l


def operand_classes(rnd, vbound, low=N_MAX, nrand=24, lo_value=0):
    """[(tag, limbs)]: the single-operand classes for the contract `limbs l[0..12] <= low, lo_value <= value < vbound`"""
    out = [("maxcol", maxlow(vbound, low))]
    vals = [0, 1, P - 1, P, P + 1, 2 * P - 1, 2 * P, vbound - 1]
    k = 4
    while k * P < vbound:
        vals += [k * P - 1, k * P, k * P + 1]
        k *= 2
    out += [("value:%d" % i, exact(v)) for i, v in enumerate(vals) if lo_value <= v < vbound]
    # non-exact spellings: a limb of 2^28 borrowed from the next one, wherever the result still respects the limb bound
    spell = []
    for v in [P, 2 * P, 1 << W, 1 << (5 * W), P + (1 << W) - C["P"][0], (1 << (13 * W)), vbound - 1] + [P + ((1 << W) - C["P"][j] << (W * j)) for j in (3, 12)]:
        if not lo_value <= v < vbound:
            continue
        e = exact(v)
        for j in range(NL - 1):
            b = borrow(e, j)
            if b is not None and b[j] <= low:
                spell.append(b)
    out += [("spell:%d" % i, l) for i, l in enumerate(spell[:12])]
    # exact values whose low limb looks like zero's or p's (the slow path of the exact zero tests)
    slow = [1 << W, (1 << W) * 12345, C["P"][0], P + (1 << W), P + (1 << (7 * W)), P - (1 << (3 * W)), C["P"][0] + (1 << (13 * W)), 2 * P - C["P"][0] - (P & ~MASK) + (1 << W)]
    out += [("slow:%d" % i, exact(v)) for i, v in enumerate(slow) if lo_value <= v < vbound]
    top = (vbound - 1) >> (W * (NL - 1))
    for par in (0, 1):
        l = [low if (j & 1) == par else 0 for j in range(NL - 1)] + [top if par else 0]
        if lo_value <= val(l) < vbound:
            out.append(("pattern:alt%d" % par, l))
    for j in range(NL):
        l = [0] * NL
        l[j] = low if j < NL - 1 else top
        if lo_value <= val(l) < vbound:
            out.append(("pattern:hot%d" % j, l))
    for i in range(nrand):
        l = rand_nform(rnd, vbound, low)
        if val(l) >= lo_value:
            out.append(("random:%d" % i, l))
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
class Vec:
    def __init__(self, tag, ins, aux=0):
        self.tag, self.ins, self.aux = tag, [list(map(int, l)) for l in ins], aux


class Out:
    """One result slot: res = residue mod p, or exact = the integer itself; value in [lo, hi); limbs 'E' exact, 'N' N-form, a per-limb
    list of exclusive bounds, or None; equal = the limbs must be exactly these"""
    def __init__(self, res=None, exact_v=None, lo=0, hi=None, limbs=None, equal=None):
        self.res, self.exact, self.lo, self.hi, self.limbs, self.equal = res, exact_v, lo, hi, limbs, equal


def check_out(name, vec, k, limbs, want):
    where = "%s [%s] result %d: " % (name, vec.tag, k)
    v = val(limbs)
    if want.equal is not None:
        assert list(limbs) == list(want.equal), where + "limbs differ from the expected ones"
    if want.exact is not None:
        assert v == want.exact, where + "value %#x, expected exactly %#x" % (v, want.exact)
    if want.res is not None:
        assert v % P == want.res % P, where + "wrong residue"
    if want.hi is not None:
        assert want.lo <= v < want.hi, where + "value %.4f p outside [%.4f p, %.4f p)" % (v / P, want.lo / P, want.hi / P)
    if want.limbs == "E":
        assert all(x <= E_MAX for x in limbs[:NL - 1]), where + "limbs not exact"
    elif want.limbs == "N":
        assert all(x <= N_MAX for x in limbs[:NL - 1]), where + "limbs above the N-form bound 2^28 + 15"
    elif want.limbs is not None:
        assert all(x < b for x, b in zip(limbs, want.limbs)), where + "limbs above the documented lazy bound"


def lowmax(l):
    return max(l[:NL - 1])


def mont(*pairs):
    return sum(val(a) * val(b) for a, b in pairs) * RINV % P


def need_mul(pairs, col_rule=None):
    """the multiplier's contract: sum of products < 2^392 p; N-form operands, or — where a comment allows lazy limbs — the column rule"""
    assert sum(val(a) * val(b) for a, b in pairs) < RP, "sum of products >= 2^392 p"
    for a, b in pairs:
        assert a[NL - 1] < 1 << 24 and b[NL - 1] < 1 << 24     # "l[13] small": a value of a few hundred p at most
    if col_rule is None:
        assert all(lowmax(a) <= N_MAX and lowmax(b) <= N_MAX for a, b in pairs), "operand not in N-form"
    else:
        assert 14 * sum(max(a) * max(b) for a, b in pairs) < col_rule, "column rule"


MUL_OUT = dict(lo=0, hi=2 * P, limbs="E")      # "Returns exact limbs, < 2p"


# ------------------------------------------------------------------------------------------------------------------------------------
# model of the column arithmetic, for the REPORT of column magnitudes only
def model_reduce(cols, signed=False):
    """fp_mont_reduce / fp_mont_reduce_signed on 28 columns: (result limbs, largest |column| seen)"""
    c = list(cols)
    peak = max(abs(x) for x in c)
    for i in range(NL):
        m = ((c[i] & 0xFFFFFFFF) * C["PINV"]) & MASK
        for j in range(NL):
            c[i + j] += m * C["P"][j]
        peak = max(peak, max(abs(x) for x in c))
        c[i + 1] += c[i] >> W
    out, carry = [], 0
    for k in range(NL):
        v = c[NL + k] + carry
        out.append(v & MASK)
        carry = v >> W
    out[NL - 1] |= (carry << W) & 0xFFFFFFFF
    return out, peak


def model_cols(pairs):
    c = [0] * (2 * NL)
    for a, b in pairs:
        for i in range(NL):
            for j in range(NL):
                c[i + j] += a[i] * b[j]
    return c


def model_mul(*pairs):
    return model_reduce(model_cols(pairs))


def model_norm(l):
    r, cp = [], 0
    for k in range(NL - 1):
        r.append((l[k] & MASK) + cp)
        cp = l[k] >> W
    return r + [l[NL - 1] + cp]


def model_add(a, b, lazy=False):
    s = [x + y for x, y in zip(a, b)]
    return s if lazy else model_norm(s)


def model_sub(K, a, b, lazy=False, wide=False):
    S = C["S8B"] if wide else C["S%d" % K]
    s = [x + t - y for x, t, y in zip(a, S, b)]
    assert all(0 <= x < 1 << 32 for x in s)
    return s if lazy else model_norm(s)


ZERO = [0] * NL


# ------------------------------------------------------------------------------------------------------------------------------------
OPS = {}          # name -> dict(gen, legal, ref, peak, family)


def op(name, family, gen, legal, ref, peak=None):
    OPS[name] = dict(gen=gen, legal=legal, ref=ref, peak=peak, family=family)


def _rnd(name):
    return random.Random("%x:%s" % (SEED, name))


def pair_up(rnd, ca, cb, extra=()):
    """vectors of a two-operand op from the operand classes of each: the maxcol corner against maxcol and against the minimal operands,
    then every class of one operand against a random one of the other"""
    vecs = []
    mins = [("min0", ZERO), ("min1", exact(1))]
    amax, bmax = ca[0], cb[0]
    vecs.append(Vec("maxcol:both", [amax[1], bmax[1]]))
    for t, m in mins:
        vecs.append(Vec("maxcol:a/" + t, [amax[1], m]))
        vecs.append(Vec("maxcol:b/" + t, [m, bmax[1]]))
    for t, l in ca[1:]:
        vecs.append(Vec(t + "/a", [l, rnd.choice(cb)[1]]))
    for t, l in cb[1:]:
        vecs.append(Vec(t + "/b", [rnd.choice(ca)[1], l]))
    return vecs + list(extra)


# ---- Fp multipliers: "a, b in N-form (limbs < 2^29.5 are still safe), a*b < 2^392 p.  Result N-form, < 2p" / exact limbs
def gen_mul(name):
    rnd = _rnd("fp_mul")      # the three forms of a multiplier share their vectors (bit-identical results are asserted)
    root = isqrt(RP - 1)
    vecs = []
    for low, t in ((N_MAX, ""), (MUL_LAZY_MAX, "lazy:")):
        ca = operand_classes(rnd, root, low, nrand=20)
        cb = operand_classes(rnd, root, low, nrand=20)
        vs = pair_up(rnd, ca, cb)
        # one operand at the top of the largest K p contract of the file (64p) against the minimal ones
        for mt, m in (("min0", ZERO), ("min1", exact(1)), ("p-1", exact(P - 1))):
            vs.append(Vec("maxcol:a64p/" + mt, [maxlow(64 * P, low), m]))
            vs.append(Vec("maxcol:b64p/" + mt, [m, maxlow(64 * P, low)]))
        for v in vs:
            v.tag = t + v.tag
        vecs += vs
    return vecs


def legal_mul(v):
    need_mul([(v.ins[0], v.ins[1])], COL_LAZY if lowmax(v.ins[0]) > N_MAX or lowmax(v.ins[1]) > N_MAX else None)
    assert max(lowmax(v.ins[0]), lowmax(v.ins[1])) <= MUL_LAZY_MAX


def ref_mul(v):
    return [Out(res=mont((v.ins[0], v.ins[1])), **MUL_OUT)], None


def peak_mul(v):
    return model_mul((v.ins[0], v.ins[1]))[1]


for _n in ("fp_mul", "fp_mul_os", "fp_mul_call"):
    op(_n, "fp_mul", gen_mul, legal_mul, ref_mul, peak_mul)


def gen_sqr(name):
    rnd = _rnd("fp_sqr")
    root = isqrt(RP - 1)
    vecs = []
    for low, t in ((N_MAX, ""), (MUL_LAZY_MAX, "lazy:")):
        vecs += [Vec(t + tag, [l]) for tag, l in operand_classes(rnd, root, low, nrand=30)]
    return vecs


op_sqr = dict(legal=lambda v: legal_mul(Vec(v.tag, [v.ins[0], v.ins[0]])),
              ref=lambda v: ([Out(res=mont((v.ins[0], v.ins[0])), **MUL_OUT)], None),
              peak=lambda v: model_mul((v.ins[0], v.ins[0]))[1])
for _n in ("fp_sqr", "fp_sqr_os", "fp_sqr_call"):
    op(_n, "fp_mul", gen_sqr, op_sqr["legal"], op_sqr["ref"], op_sqr["peak"])


# fp_mul2add: "(a*b + c*d) / 2^392 mod p with ONE Montgomery reduction (28 + 14 terms of < 2^56 stay below 2^62).  Needs a*b + c*d < 2^392 p"
# lazy operands: CoopF2::neg32_lazy "32p - b without a carry pass (b in N-form, < 31p): limbs < 2^29, still a legal multiplier operand next
# to N-form partners"; the hot loop's Y3 = mul2add(t1, t2, ny, t0) with t1, t2, ny one lazy subtraction each (limbs < 2^29 + 68 above
# an exact operand's, tools/bounds_check.py check_madd_lazy) and t0 exact.
def lazy_neg(K, b):
    return [s - x for s, x in zip(C["S%d" % K], b)]


def gen_mulNadd(n_pairs, name):
    rnd = _rnd("fp_mul%dadd" % n_pairs)
    each = isqrt((RP - 1) // n_pairs)
    vecs = []
    cls = [operand_classes(rnd, each, N_MAX, nrand=10) for _ in range(2 * n_pairs)]
    mx = [c[0][1] for c in cls]
    vecs.append(Vec("maxcol:all", mx))
    for i in range(2 * n_pairs):       # each operand alone at its corner, the others minimal
        vecs.append(Vec("maxcol:%d/min0" % i, [mx[j] if j == i else ZERO for j in range(2 * n_pairs)]))
        vecs.append(Vec("maxcol:%d/min1" % i, [mx[j] if j == i else exact(1) for j in range(2 * n_pairs)]))
    for i in range(2 * n_pairs):
        for t, l in cls[i][1:]:
            vecs.append(Vec("%s/%d" % (t, i), [l if j == i else rnd.choice(cls[j])[1] for j in range(2 * n_pairs)]))
    # second operand of every second product lazily negated: 32p - b, b at the N-form corner below 31p, at 0, at random
    for t, b in (("max", maxlow(31 * P)), ("zero", ZERO), ("rand", rand_nform(rnd, 31 * P))):
        nb = lazy_neg(32, b)
        a = maxlow((RP - 1) // n_pairs // val(nb) + 1 if val(nb) * val(mx[0]) * n_pairs >= RP else each)
        ins = []
        for q in range(n_pairs):
            ins += [a, nb if q & 1 else maxlow(min(each, (RP - 1) // n_pairs // val(a)))]
        vecs.append(Vec("maxcol:neg32_lazy:" + t, ins))
    if n_pairs == 2:                   # the hot loop's limb classes: R (Q - X3) + (8p - Y1) PPP at R < 10p, Q - X3 < 18p, 8p - Y1 < 8p, PPP < 2p
        hi = (1 << 28) - 1 + SUB_LAZY_GROW - 1
        vecs.append(Vec("maxcol:hotloop", [maxlow(10 * P, hi), maxlow(18 * P, hi), maxlow(8 * P, hi), maxlow(2 * P, E_MAX)]))
        for i in range(10):
            vecs.append(Vec("random:hotloop%d" % i, [rand_nform(rnd, 10 * P, hi), rand_nform(rnd, 18 * P, hi), rand_nform(rnd, 8 * P, hi), rand_nform(rnd, 2 * P, E_MAX)]))
    return vecs


def _pairs(v):
    return [(v.ins[2 * q], v.ins[2 * q + 1]) for q in range(len(v.ins) // 2)]


def legal_mulNadd(v):
    lazy = any(lowmax(l) > N_MAX for l in v.ins)
    need_mul(_pairs(v), COL_LAZY if lazy else None)
    assert all(lowmax(l) <= (1 << 28) - 1 + SUB_LAZY_GROW for l in v.ins)


for _n, _k in (("fp_mul2add", 2), ("fp_mul2add_os", 2), ("fp_mul2add_call", 2), ("fp_mul4add", 4)):
    op(_n, "fp_mul", (lambda name, k=_k: gen_mulNadd(k, name)), legal_mulNadd,
       lambda v: ([Out(res=mont(*_pairs(v)), **MUL_OUT)], None), lambda v: model_mul(*_pairs(v))[1])


# ---- linear ops
BIG = 127 * P      # the largest value contract of the file (fp_reduce_small: "N-form value v < 127p")


def gen_add(name):
    rnd = _rnd("fp_add")
    vecs = pair_up(rnd, operand_classes(rnd, BIG), operand_classes(rnd, BIG))
    # fp_norm1: "any limbs < 2^32 -> N-form": limb sums right below 2^32
    w = (1 << 31) - 1
    vecs += [Vec("maxcol:wide", [maxlow(BIG, w), maxlow(BIG, w)]), Vec("maxcol:wide/min", [maxlow(BIG, (1 << 32) - 1), ZERO]),
             Vec("pattern:wide", [[w, 0] * 6 + [w, 5], [w, 1] * 6 + [w, 7]])]
    vecs += [Vec("random:wide%d" % i, [rand_nform(rnd, BIG, w), rand_nform(rnd, BIG, w)]) for i in range(16)]
    return vecs


def legal_add(v):
    a, b = v.ins
    assert all(x + y < 1 << 32 for x, y in zip(a, b)) and a[13] + b[13] + 16 < 1 << 32


op("fp_add", "fp_linear", gen_add, legal_add, lambda v: ([Out(exact_v=val(v.ins[0]) + val(v.ins[1]), limbs="N")], None))
op("fp_add_lazy", "fp_linear", gen_add, legal_add,
   lambda v: ([Out(exact_v=val(v.ins[0]) + val(v.ins[1]), equal=[x + y for x, y in zip(*v.ins)])], None))


def gen_norm(name):
    rnd = _rnd("fp_norm")
    vecs = []
    for low, t in ((N_MAX, ""), ((1 << 32) - 1, "wide:"), (WIDE_MAX + SUB_LAZY_GROW, "lazy:")):
        vecs += [Vec(t + tag, [l]) for tag, l in operand_classes(rnd, BIG, low, nrand=16)]
    return vecs


op("fp_norm", "fp_linear", gen_norm, lambda v: legal_add(Vec(v.tag, [v.ins[0], ZERO])), lambda v: ([Out(exact_v=val(v.ins[0]), limbs="N")], None))


# fp_sub<K>: "r = a - b + K*p, K in {2,4,8,16,32,64}; requires b in N-form with value < (K-1)p. Result < a + K*p"
# fp_sub_lazy<K>: "b must have limbs <= SPREAD_LO (exact / N-form) and value < (K-1) p; result limbs < a + 2^29 + 68"
def gen_sub(K, lazy, name):
    rnd = _rnd("fp_sub%d%s" % (K, "l" if lazy else ""))
    blow = SPREAD_LO if lazy else N_MAX
    cb = operand_classes(rnd, (K - 1) * P, blow, nrand=12)
    ca = operand_classes(rnd, 64 * P, N_MAX, nrand=12)
    vecs = pair_up(rnd, ca, cb)
    if lazy:    # a minuend that is itself lazy: limbs up to 2^32 - (2^29 + 68)
        wide = (1 << 32) - SUB_LAZY_GROW
        vecs += [Vec("maxcol:lazy_a", [maxlow(64 * P, wide), cb[0][1]]), Vec("maxcol:lazy_a/min", [maxlow(64 * P, wide), ZERO])]
    return vecs


def legal_sub(K, lazy, v):
    a, b = v.ins
    assert lowmax(b) <= (SPREAD_LO if lazy else N_MAX) and val(b) < (K - 1) * P
    assert all(x + SUB_LAZY_GROW <= 1 << 32 for x in a[:13]) and a[13] < 1 << 24


def ref_sub(K, lazy, v):
    a, b = v.ins
    want = val(a) - val(b) + K * P
    if lazy:
        return [Out(exact_v=want, limbs=[x + SUB_LAZY_GROW for x in a[:13]] + [1 << 32])], None
    return [Out(exact_v=want, limbs="N")], None


for _K in (2, 4, 8, 16, 32, 64):
    op("fp_sub%d" % _K, "fp_linear", (lambda name, K=_K: gen_sub(K, False, name)), (lambda v, K=_K: legal_sub(K, False, v)), (lambda v, K=_K: ref_sub(K, False, v)))
    op("fp_sub_lazy%d" % _K, "fp_linear", (lambda name, K=_K: gen_sub(K, True, name)), (lambda v, K=_K: legal_sub(K, True, v)), (lambda v, K=_K: ref_sub(K, True, v)))
    op("fp_neg%d" % _K, "fp_linear", (lambda name, K=_K: [Vec(t, [l]) for t, l in operand_classes(_rnd("fp_neg%d" % K), (K - 1) * P, nrand=16)]),
       (lambda v, K=_K: legal_sub(K, False, Vec(v.tag, [ZERO, v.ins[0]]))), (lambda v, K=_K: ([Out(exact_v=K * P - val(v.ins[0]), limbs="N")], None)))


# fp_sub8_lazy_wide: "a - b + 8p where b is a lazy sum of up to three exact values (limbs < 3 * 2^28)"; S8B: "value < 7p"
def gen_sub8w(name):
    rnd = _rnd(name)
    cb = operand_classes(rnd, 7 * P, WIDE_MAX, nrand=16)
    ca = operand_classes(rnd, 2 * P, E_MAX, nrand=16)      # the hot loop's minuend is a square: exact, < 2p
    return pair_up(rnd, ca, cb) + [Vec("maxcol:nform_a", [maxlow(64 * P), cb[0][1]])]


def legal_sub8w(v):
    a, b = v.ins
    assert lowmax(b) <= WIDE_MAX and val(b) < 7 * P and lowmax(a) <= N_MAX and a[13] < 1 << 24


op("fp_sub8_lazy_wide", "fp_linear", gen_sub8w, legal_sub8w,
   lambda v: ([Out(exact_v=val(v.ins[0]) - val(v.ins[1]) + 8 * P, limbs=[x + (1 << 30) + 68 for x in v.ins[0][:13]] + [1 << 32])], None))


# fp_mul_small<K>: "r = K*a for a small constant K (K * limb must stay below 2^32: K <= 15)"
def gen_mul_small(K, name):
    rnd = _rnd(name)
    vecs = []
    for low, t in ((N_MAX, ""), (((1 << 32) - 1) // K, "wide:")):
        vecs += [Vec(t + tag, [l]) for tag, l in operand_classes(rnd, 64 * P, low, nrand=16)]
    return vecs


for _K in (2, 3, 12, 15):
    op("fp_mul_small%d" % _K, "fp_linear", (lambda name, K=_K: gen_mul_small(K, name)),
       (lambda v, K=_K: legal_add(Vec(v.tag, [[K * x for x in v.ins[0]], ZERO]))), (lambda v, K=_K: ([Out(exact_v=K * val(v.ins[0]), limbs="N")], None)))


# ---- reductions and predicates
# fp_reduce_small: "for an N-form value v < 127p: result N-form, p <= result < 2.01p"
def gen_reduce_small(name):
    rnd = _rnd(name)
    vecs = [Vec(t, [l]) for t, l in operand_classes(rnd, BIG, nrand=40)]
    for m in range(0, 127):        # every multiple up to 126: right below (m + 1) p with maximal low limbs, and m p itself
        vecs.append(Vec("maxcol:%dp" % (m + 1), [maxlow((m + 1) * P)]))
        vecs.append(Vec("value:%dp" % m, [exact(m * P)]))
    return vecs


def legal_nform(bound, v, low=N_MAX):
    assert all(lowmax(l) <= low and val(l) < bound for l in v.ins)


op("fp_reduce_small", "fp_reduce", gen_reduce_small, lambda v: legal_nform(BIG, v),
   lambda v: ([Out(res=val(v.ins[0]), lo=P, hi=2 * P + P // 100, limbs="N")], None))


def gen_one(bound, low, name, nrand=24):
    return [Vec(t, [l]) for t, l in operand_classes(_rnd(name), bound, low, nrand=nrand)]


# fp_carry_exact: "Exact carry propagation of an N-form value that fits 392 bits: limbs -> [0, 2^28), l[13] holds the rest"
op("fp_carry_exact", "fp_reduce", lambda name: gen_one(BIG, N_MAX, name), lambda v: legal_nform(BIG, v),
   lambda v: ([Out(exact_v=val(v.ins[0]), limbs="E")], None))
# fp_canon_2p: "Canonical representative in [0, p) with exact 28-bit limbs, for an N-form value < 2p"
op("fp_canon_2p", "fp_reduce", lambda name: gen_one(2 * P, N_MAX, name), lambda v: legal_nform(2 * P, v),
   lambda v: ([Out(exact_v=val(v.ins[0]) % P, limbs="E")], None))
# fp_is_zero_2p: "a == 0 (mod p) for an N-form value < 2p"; _exact: "The same for a value with EXACT limbs"; _any: "any N-form value < ~50p"
op("fp_is_zero_2p", "fp_reduce", lambda name: gen_one(2 * P, N_MAX, name), lambda v: legal_nform(2 * P, v),
   lambda v: ([Out(equal=ZERO)], int(val(v.ins[0]) % P == 0)))
op("fp_is_zero_2p_exact", "fp_reduce", lambda name: gen_one(2 * P, E_MAX, name), lambda v: legal_nform(2 * P, v, E_MAX),
   lambda v: ([Out(equal=ZERO)], int(val(v.ins[0]) % P == 0)))
op("fp_is_zero_any", "fp_reduce", lambda name: gen_one(50 * P, N_MAX, name), lambda v: legal_nform(50 * P, v),
   lambda v: ([Out(equal=ZERO)], int(val(v.ins[0]) % P == 0)))


# ------------------------------------------------------------------------------------------------------------------------------------
# Fp2 = Fp[u] / (u^2 + 1), one lane (ec::Fp2Ops "fp2c", ec::Fp2OpsInline "fp2i") and lane pair (CoopF2 / CoopF2A): same vectors, so the
# lane-pair results can be compared with the one-lane ones.  ec.cuh:
#   "c0 = a0 b0 + a1 (32p - b1)   needs b1 <= 31p and a (b + 32) < 2^392/p ~ 2520;   c1 = a0 b1 + a1 b0   needs 2 a b < 2520"
def f2(l0, l1):
    return (val(l0), val(l1))


def f2mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def distinct_max(bound, low=N_MAX):
    """the maxcol corner for the two components of an Fp2 value, kept distinct (a wrong lane-pair partner must show)"""
    a = maxlow(bound, low)
    b = list(a)
    b[NL - 1] -= 1
    b[5] -= 3
    return a, b


def fp2_classes(rnd, bound, low=N_MAX, nrand=10, lo_value=0):
    c0 = operand_classes(rnd, bound, low, nrand, lo_value)
    c1 = operand_classes(rnd, bound, low, nrand, lo_value)
    mx = distinct_max(bound, low)
    out = [("maxcol", mx[0], mx[1]), ("maxcol:c0", mx[0], ZERO), ("maxcol:c1", ZERO, mx[1])]
    out += [(t + "/c0", l, rnd.choice(c1)[1]) for t, l in c0[1:]]
    out += [(t + "/c1", rnd.choice(c0)[1], l) for t, l in c1[1:]]
    return out


def legal_fp2_mul(a0, a1, b0, b1):
    assert val(b1) < 31 * P and val(b0) < 31 * P
    nb1 = 32 * P - val(b1)
    assert val(a0) * val(b0) + val(a1) * nb1 < RP and val(a0) * val(b1) + val(a1) * val(b0) < RP
    assert all(lowmax(l) <= N_MAX and l[13] < 1 << 24 for l in (a0, a1, b0, b1))


def gen_fp2_mul(name):
    rnd = _rnd("fp2_mul")
    bb = 31 * P                                   # "b1 <= 31p"
    ab = (RP - 1) // (63 * P)                     # a (b + 32) < 2^392 / p at b = 31p
    ca, cb = fp2_classes(rnd, ab), fp2_classes(rnd, bb)
    vecs = [Vec("maxcol:both", [ca[0][1], ca[0][2], cb[0][1], cb[0][2]])]
    for t, x0, x1 in ca[:3]:
        for mt, m in (("min0", ZERO), ("min1", exact(1))):
            vecs.append(Vec("%s:a/%s" % (t, mt), [x0, x1, m, m]))
    for t, x0, x1 in cb[:3]:
        for mt, m in (("min0", ZERO), ("min1", exact(1))):
            vecs.append(Vec("%s:b/%s" % (t, mt), [m, m, x0, x1]))
    for t, x0, x1 in ca[3:]:
        y = rnd.choice(cb)
        vecs.append(Vec(t + "/a", [x0, x1, y[1], y[2]]))
    for t, x0, x1 in cb[3:]:
        y = rnd.choice(ca)
        vecs.append(Vec(t + "/b", [y[1], y[2], x0, x1]))
    rnd.shuffle(vecs)                             # neighbouring lane pairs of a wave carry different classes
    return vecs


def model_fp2_mul_peak(a0, a1, b0, b1, lazy_neg32):
    nb1 = lazy_neg(32, b1) if lazy_neg32 else model_sub(32, ZERO, b1)
    return max(model_mul((a0, b0), (a1, nb1))[1], model_mul((a0, b1), (a1, b0))[1])


def ref_fp2_mul(v):
    r = f2mul(f2(*v.ins[0:2]), f2(*v.ins[2:4]))
    return [Out(res=r[0] * RINV, **MUL_OUT), Out(res=r[1] * RINV, **MUL_OUT)], None


# sqr: "(a0 + a1)(a0 - a1) + 2 a0 a1 u ; a < 22p"; the lane-pair squaring "takes components below 20p only" (ec.cuh jac_dbl)
def gen_fp2_sqr(bound, name):
    rnd = _rnd("fp2_sqr")
    vecs = [Vec(t, [x0, x1]) for t, x0, x1 in fp2_classes(rnd, bound, nrand=16)]
    rnd.shuffle(vecs)
    return vecs


def ref_fp2_sqr(v):
    a = f2(*v.ins)
    r = f2mul(a, a)
    return [Out(res=r[0] * RINV, **MUL_OUT), Out(res=r[1] * RINV, **MUL_OUT)], None


def peak_fp2_sqr(v):
    a0, a1 = v.ins
    return max(model_mul((model_add(a0, a1), model_sub(32, a0, a1)))[1], model_mul((model_add(a0, a0), a1))[1])


# mul2add: "a b + c d ; b, d <= 31p", the inlined forms as ONE four-product reduction (< 2p, exact), the shared-call and the plain CoopF2
# forms as the sum of two products (N-form, < 4p)
def gen_fp2_mul2add(name):
    rnd = _rnd("fp2_mul2add")
    bb = 31 * P
    ab = (RP - 1) // (2 * 63 * P)
    ca, cb = fp2_classes(rnd, ab, nrand=8), fp2_classes(rnd, bb, nrand=8)
    mxa, mxb = ca[0], cb[0]
    vecs = [Vec("maxcol:all", [mxa[1], mxa[2], mxb[1], mxb[2], mxa[2], mxa[1], mxb[2], mxb[1]])]
    vecs.append(Vec("maxcol:first/min", [mxa[1], mxa[2], mxb[1], mxb[2], ZERO, ZERO, ZERO, ZERO]))
    vecs.append(Vec("maxcol:second/min", [exact(1), ZERO, exact(1), ZERO, mxa[1], mxa[2], mxb[1], mxb[2]]))
    for i, cls in enumerate((ca, cb, ca, cb)):
        for t, x0, x1 in cls[1:]:
            ins = []
            for j, other in enumerate((ca, cb, ca, cb)):
                y = (t, x0, x1) if i == j else rnd.choice(other)
                ins += [y[1], y[2]]
            vecs.append(Vec("%s/%d" % (t, i), ins))
    rnd.shuffle(vecs)
    return vecs


def legal_fp2_mul2add(v):
    a0, a1, b0, b1, c0, c1, d0, d1 = v.ins
    legal_fp2_mul(a0, a1, b0, b1)
    legal_fp2_mul(c0, c1, d0, d1)
    nb1, nd1 = 32 * P - val(b1), 32 * P - val(d1)
    assert val(a0) * val(b0) + val(a1) * nb1 + val(c0) * val(d0) + val(c1) * nd1 < RP
    assert val(a0) * val(b1) + val(a1) * val(b0) + val(c0) * val(d1) + val(c1) * val(d0) < RP


def ref_fp2_mul2add(fused, v):
    x, y = f2mul(f2(*v.ins[0:2]), f2(*v.ins[2:4])), f2mul(f2(*v.ins[4:6]), f2(*v.ins[6:8]))
    form = MUL_OUT if fused else dict(lo=0, hi=4 * P, limbs="N")
    return [Out(res=(x[0] + y[0]) * RINV, **form), Out(res=(x[1] + y[1]) * RINV, **form)], None


def peak_fp2_mul2add(lazy_neg32, v):
    a0, a1, b0, b1, c0, c1, d0, d1 = v.ins
    nb1, nd1 = (lazy_neg(32, b1), lazy_neg(32, d1)) if lazy_neg32 else (model_sub(32, ZERO, b1), model_sub(32, ZERO, d1))
    return max(model_mul((a0, b0), (a1, nb1), (c0, d0), (c1, nd1))[1], model_mul((a0, b1), (a1, b0), (c0, d1), (c1, d0))[1])


# sqr_sub12sqr: "s^2 - 12 e^2 ... s <= 22p, e < 3p; result < 2p"
def gen_fp2_ss(name):
    rnd = _rnd("fp2_sqr_sub12sqr")
    cs, ce = fp2_classes(rnd, 22 * P, nrand=10), fp2_classes(rnd, 3 * P, nrand=10)
    vecs = [Vec("maxcol:both", [cs[0][1], cs[0][2], ce[0][1], ce[0][2]]), Vec("maxcol:s/min", [cs[0][1], cs[0][2], ZERO, ZERO]),
            Vec("maxcol:e/min", [ZERO, ZERO, ce[0][1], ce[0][2]])]
    for t, x0, x1 in cs[1:]:
        y = rnd.choice(ce)
        vecs.append(Vec(t + "/s", [x0, x1, y[1], y[2]]))
    for t, x0, x1 in ce[1:]:
        y = rnd.choice(cs)
        vecs.append(Vec(t + "/e", [y[1], y[2], x0, x1]))
    rnd.shuffle(vecs)
    return vecs


def legal_fp2_ss(v):
    s0, s1, e0, e1 = v.ins
    assert all(val(l) < 22 * P for l in (s0, s1)) and all(val(l) < 3 * P for l in (e0, e1)) and all(lowmax(l) <= N_MAX for l in v.ins)


def ref_fp2_ss(v):
    s, e = f2(*v.ins[0:2]), f2(*v.ins[2:4])
    ss, ee = f2mul(s, s), f2mul(e, e)
    return [Out(res=(ss[0] - 12 * ee[0]) * RINV, **MUL_OUT), Out(res=(ss[1] - 12 * ee[1]) * RINV, **MUL_OUT)], None


# mul_b3: b3 = 12 (1 + u) as a field product with the constant TWELVE (= 12 * 2^392 mod p: the product IS 12 a in the same domain);
# one lane: a product by (TWELVE, TWELVE), the contract of mul; lane pair: "a <= 3p, result < 2p"
assert val(C["TWELVE"]) == 12 * R % P and val(C["ONE"]) == R % P


def gen_fp2_b3(name):
    rnd = _rnd("fp2_mul_b3")
    vecs = [Vec(t, [x0, x1]) for t, x0, x1 in fp2_classes(rnd, 3 * P, nrand=16)]
    rnd.shuffle(vecs)
    return vecs


def ref_fp2_b3(v):
    a = f2(*v.ins)
    return [Out(res=12 * (a[0] - a[1]), **MUL_OUT), Out(res=12 * (a[0] + a[1]), **MUL_OUT)], None


# is_zero_2p of an Fp2 value: both components; the lane-pair form takes "a multiplier output (exact limbs)"
def gen_fp2_zero(name):
    rnd = _rnd("fp2_is_zero")
    zeros = [ZERO, exact(P)]
    xs = [exact(7), exact(P + 1), exact(1 << W), exact(C["P"][0]), exact(P + (1 << (4 * W))), exact(2 * P - 1)] + [exact(rnd.randrange(2 * P)) for _ in range(8)]
    vecs = [Vec("value:(%s,%s)" % ("0p"[i], "0p"[j]), [zeros[i], zeros[j]]) for i in (0, 1) for j in (0, 1)]
    for i, x in enumerate(xs):
        for zi, z in enumerate(zeros):
            vecs += [Vec("slow:(%s,x%d)" % ("0p"[zi], i), [z, x]), Vec("slow:(x%d,%s)" % (i, "0p"[zi]), [x, z])]
        vecs.append(Vec("random:(x,x)%d" % i, [x, xs[(i + 1) % len(xs)]]))
    rnd.shuffle(vecs)
    return vecs


def ref_fp2_zero(v):
    return [Out(equal=ZERO)], int(val(v.ins[0]) % P == 0 and val(v.ins[1]) % P == 0)


for _v in ("fp2c", "fp2i"):
    op(_v + "_mul", "fp2_lane", gen_fp2_mul, lambda v: legal_fp2_mul(*v.ins), ref_fp2_mul, lambda v: model_fp2_mul_peak(*v.ins, False))
    op(_v + "_sqr", "fp2_lane", lambda name: gen_fp2_sqr(20 * P, name), lambda v: legal_nform(22 * P, v), ref_fp2_sqr, peak_fp2_sqr)
    op(_v + "_mul2add", "fp2_lane", gen_fp2_mul2add, legal_fp2_mul2add, (lambda v, f=(_v == "fp2i"): ref_fp2_mul2add(f, v)), lambda v: peak_fp2_mul2add(False, v))
    op(_v + "_sqr_sub12sqr", "fp2_lane", gen_fp2_ss, legal_fp2_ss, ref_fp2_ss)
    op(_v + "_mul_b3", "fp2_lane", gen_fp2_b3, lambda v: legal_fp2_mul(v.ins[0], v.ins[1], C["TWELVE"], C["TWELVE"]), ref_fp2_b3)
    op(_v + "_is_zero_2p", "fp2_lane", gen_fp2_zero, lambda v: legal_nform(2 * P, v), ref_fp2_zero)

op("coop_mul", "coop", gen_fp2_mul, lambda v: legal_fp2_mul(*v.ins), ref_fp2_mul, lambda v: model_fp2_mul_peak(*v.ins, True))
op("coop_sqr", "coop", lambda name: gen_fp2_sqr(20 * P, name), lambda v: legal_nform(20 * P, v), ref_fp2_sqr, peak_fp2_sqr)
op("coop_sqr_sub12sqr", "coop", gen_fp2_ss, legal_fp2_ss, ref_fp2_ss)
op("coop_mul2add", "coop", gen_fp2_mul2add, legal_fp2_mul2add, lambda v: ref_fp2_mul2add(False, v))
op("coop_mul_b3", "coop", gen_fp2_b3, lambda v: legal_nform(3 * P, v), ref_fp2_b3)
op("coop_one", "coop", lambda name: [Vec("value:%d" % i, [exact(i), exact(99 - i)]) for i in range(70)], lambda v: None,
   lambda v: ([Out(equal=C["ONE"]), Out(equal=ZERO)], None))
op("coopa_mul2add", "coop", gen_fp2_mul2add, legal_fp2_mul2add, lambda v: ref_fp2_mul2add(True, v), lambda v: peak_fp2_mul2add(True, v))
op("coopa_is_zero_2p", "coop", gen_fp2_zero, lambda v: legal_nform(2 * P, v, E_MAX), lambda v: ([Out(equal=ZERO), Out(equal=ZERO)], ref_fp2_zero(v)[1]))


def gen_all_zero(name):
    rnd = _rnd(name)
    vecs = [Vec("value:(0,0)", [ZERO, ZERO]), Vec("value:(p,p)", [exact(P), exact(P)]), Vec("value:(0,p)", [ZERO, exact(P)]), Vec("value:(p,0)", [exact(P), ZERO])]
    for j in range(NL):
        hot = [0] * NL
        hot[j] = 1 << rnd.randrange(28)
        vecs += [Vec("pattern:hot%d/c0" % j, [hot, ZERO]), Vec("pattern:hot%d/c1" % j, [ZERO, hot])]
    rnd.shuffle(vecs)
    return vecs


op("coopa_limbs_all_zero", "coop", gen_all_zero, lambda v: None,
   lambda v: ([Out(equal=ZERO), Out(equal=ZERO)], int(not any(v.ins[0]) and not any(v.ins[1]))))


# ------------------------------------------------------------------------------------------------------------------------------------
# Pairing accumulators (pairing_kernels.cuh).  KaraCols: "Operand bounds: a' <= (12p, 8p) in N-form, g <= 6p in N-form ... <= 4 terms",
# a' = a or xi a = (a0 - a1 + 8p, a0 + a1); the bias p 2^388 must cover V1 = sum a1' g1: "<= 144 p^2".  aux = terms | wrapped << 8.
def xi_values(a0, a1, wrapped, K=8):
    return (a0 - a1 + K * P, a0 + a1) if wrapped else (a0, a1)


def kara_terms(v):
    n = v.aux & 0xFF
    return [(v.ins[4 * t: 4 * t + 4], (v.aux >> (8 + t)) & 1) for t in range(n)]


def legal_kara(v, pre=False):
    terms = kara_terms(v)
    assert 1 <= len(terms) <= 4
    v1 = 0
    for (a0, a1, g0, g1), w in terms:
        assert all(lowmax(l) <= N_MAX for l in (a0, a1, g0, g1))
        if pre:    # lds_store_variants: "f exact (< 2p per component): s < 4p, d < 6p, d + s < 10p"
            assert all(lowmax(l) <= E_MAX and val(l) < 2 * P for l in (a0, a1))
        if w:
            assert val(a1) < (3 if pre else 7) * P     # the subtrahend of fp_sub<4> / fp_sub<8>
        x0, x1 = xi_values(val(a0), val(a1), w, 4 if pre else 8)
        assert x0 <= 12 * P and x1 <= 8 * P and val(g0) <= 6 * P and val(g1) <= 6 * P
        v1 += x1 * val(g1)
    assert v1 <= 144 * P * P


def ref_kara(v, K=8):
    c0 = c1 = 0
    for (a0, a1, g0, g1), w in kara_terms(v):
        x0, x1 = xi_values(val(a0), val(a1), w, K)
        c0 += x0 * val(g0) - x1 * val(g1)
        c1 += x0 * val(g1) + x1 * val(g0)
    return [Out(res=c0 * RINV, **MUL_OUT), Out(res=c1 * RINV, **MUL_OUT)], None


def model_kara(v, pre=False):
    """the column arithmetic of fp2_acc_term(_pre) + fp2_kara_reduce restated: (c0 limbs, c1 limbs, largest |column|)"""
    v0, v1, v2 = [0] * 28, [0] * 28, [0] * 28
    for (a0, a1, g0, g1), w in kara_terms(v):
        if w:
            a0, a1 = model_sub(4 if pre else 8, a0, a1), model_add(a0, a1)
        s = model_add(a0, a1)
        for cols, x, y in ((v0, a0, g0), (v1, a1, g1), (v2, s, model_add(g0, g1, lazy=True))):
            for k, c in enumerate(model_cols([(x, y)])):
                cols[k] += c
    c0 = [x - y for x, y in zip(v0, v1)]
    for j in range(NL):
        c0[NL - 1 + j] += C["P"][j] << 24
    c1 = [z - x - y for x, y, z in zip(v0, v1, v2)]
    (r0, p0), (r1, p1) = model_reduce(c0, True), model_reduce(c1, True)
    return r0, r1, max(p0, p1)


def peak_kara(v, pre=False):
    return model_kara(v, pre)[2]


def kara_vec(tag, terms):
    ins, aux = [], len(terms)
    for t, ((a0, a1, g0, g1), w) in enumerate(terms):
        ins += [a0, a1, g0, g1]
        aux |= int(w) << (8 + t)
    while len(ins) < 16:
        ins.append(ZERO)
    return Vec(tag, ins, aux)


def gen_kara(pre, name):
    rnd = _rnd("kara_pre" if pre else "kara")
    lo = [0] * NL
    if pre:       # operands read from the five-value record of an exact coefficient f < 2p; g: a line's c0 <= 6p
        amax = (maxlow(2 * P, E_MAX), maxlow(2 * P, E_MAX))
        profiles = {"line": (3, amax, 6 * P + 1)}
        a_cls = lambda: operand_classes(rnd, 2 * P, E_MAX, nrand=6)
    else:         # the two users of tests/test_host_model.py: squaring (four terms, a' <= (12p, 8p), g < 2p), line (three terms, a' <= (10p, 4p), g <= 6p)
        profiles = {"square": (4, (maxlow(12 * P + 1), maxlow(8 * P + 1)), 2 * P), "line": (3, (maxlow(10 * P + 1), maxlow(4 * P + 1)), 6 * P + 1)}
        a_cls = lambda: operand_classes(rnd, 4 * P + 1, N_MAX, nrand=6)
    vecs = []
    half = [1 << 27] * 13 + [0]                    # a0 + a1 has every limb 2^28: the normalised sum differs most from the column-wise one
    for pname, (nt, amx, gb) in profiles.items():
        gmx = maxlow(gb)
        for T in range(1, nt + 1):
            # every operand at its corner (unwrapped: a' = a), the largest columns of all three sets
            vecs.append(kara_vec("maxcol:%s:T%d" % (pname, T), [((amx[0], amx[1], gmx, gmx), 0)] * T))
            # most negative c0 columns: V0 minimal, V1 maximal; and the reverse
            vecs.append(kara_vec("neg:%s:c0-:T%d" % (pname, T), [((lo, amx[1], lo, gmx), 0)] * T))
            vecs.append(kara_vec("neg:%s:c0+:T%d" % (pname, T), [((amx[0], lo, gmx, lo), 0)] * T))
            vecs.append(kara_vec("neg:%s:cross:T%d" % (pname, T), [((amx[0], lo, lo, gmx), 0)] * T))
            # wrapped terms at the corner of a: xi a = (a0 - a1 + 8p, a0 + a1) from a <= 4p (records: d = f0 - f1 + 4p from f < 2p)
            wa = maxlow(2 * P, E_MAX) if pre else maxlow(4 * P + 1)
            gw = maxlow(min(gb, (144 * P * P) // (T * 2 * val(wa)) + 1))
            vecs.append(kara_vec("maxcol:%s:wrapped:T%d" % (pname, T), [((wa, wa, gmx, gw), 1)] * T))
            vecs.append(kara_vec("neg:%s:wrapped:T%d" % (pname, T), [((wa, lo, gmx, lo), 1), ((lo, wa, lo, gw), 1)][:T] * ((T + 1) // 2) if T > 1 else [((lo, wa, lo, gw), 1)]))
            if not pre:
                vecs.append(kara_vec("neg:%s:normsum:T%d" % (pname, T), [((half, half, gmx, gmx), 0)] * T))
                vecs.append(kara_vec("neg:%s:normsum_g:T%d" % (pname, T), [((amx[0], amx[1], half, half), 0)] * T))
    # V1 right at the bias' documented cover 144 p^2: three terms of a1' = 8p against g1 = 6p (not possible from a record: s < 4p)
    if not pre:
        vecs.append(kara_vec("value:V1=144p^2", [((lo, exact(8 * P), lo, exact(6 * P)), 0)] * 3))
        vecs.append(kara_vec("maxcol:V1=144p^2", [((lo, maxlow(8 * P + 1), lo, maxlow(6 * P + 1)), 0)] * 3))
    # zero in both representations, mixed wrapped flags, random
    zs = [ZERO, exact(P)]
    for i in range(4):
        vecs.append(kara_vec("value:zero%d" % i, [((zs[i & 1], zs[i >> 1], exact(5), exact(P + 3)), i & 1), ((exact(9), exact(2), zs[i >> 1], zs[i & 1]), 1)]))
    ac = a_cls()
    gc = operand_classes(rnd, 2 * P, N_MAX, nrand=6)
    for i in range(60):
        T = 1 + i % 4
        terms = [((rnd.choice(ac)[1], rnd.choice(ac)[1], rnd.choice(gc)[1], rnd.choice(gc)[1]), rnd.randrange(2)) for _ in range(T)]
        vecs.append(kara_vec("random:%d" % i, terms))
    rnd.shuffle(vecs)
    return vecs


op("kara", "kara", lambda name: gen_kara(False, name), legal_kara, ref_kara, peak_kara)
op("kara_pre", "kara", lambda name: gen_kara(True, name), lambda v: legal_kara(v, True), lambda v: ref_kara(v, 4), lambda v: peak_kara(v, True))


# fp2_acc_term4: "a <= 4p, g exact (< 2p): xi a <= (12p, 8p) in N-form, 4p - g1 <= 4p ... six terms per reduction"
def legal_acc4(v):
    n = v.aux & 0xFF
    assert 1 <= n <= 6
    for t in range(n):
        a0, a1, g0, g1 = v.ins[4 * t: 4 * t + 4]
        assert all(lowmax(l) <= N_MAX and val(l) <= 4 * P for l in (a0, a1)) and all(lowmax(l) <= E_MAX and val(l) < 2 * P for l in (g0, g1))


def ref_acc4(v):
    c0 = c1 = 0
    for t in range(v.aux & 0xFF):
        a0, a1, g0, g1 = v.ins[4 * t: 4 * t + 4]
        x0, x1 = xi_values(val(a0), val(a1), (v.aux >> (8 + t)) & 1)
        c0 += x0 * val(g0) - x1 * val(g1)
        c1 += x0 * val(g1) + x1 * val(g0)
    return [Out(res=c0 * RINV, **MUL_OUT), Out(res=c1 * RINV, **MUL_OUT)], None


def model_acc4(v):
    p0, p1 = [], []
    for t in range(v.aux & 0xFF):
        a0, a1, g0, g1 = v.ins[4 * t: 4 * t + 4]
        if (v.aux >> (8 + t)) & 1:
            a0, a1 = model_sub(8, a0, a1), model_add(a0, a1)
        p0 += [(a0, g0), (a1, model_sub(4, ZERO, g1))]
        p1 += [(a0, g1), (a1, g0)]
    (r0, k0), (r1, k1) = model_mul(*p0), model_mul(*p1)
    return r0, r1, max(k0, k1)


def peak_acc4(v):
    return model_acc4(v)[2]


def gen_acc4(name):
    rnd = _rnd(name)
    amx, gmx, lo = maxlow(4 * P + 1), maxlow(2 * P, E_MAX), [0] * NL

    def vec(tag, terms):
        ins, aux = [], len(terms)
        for t, (q, w) in enumerate(terms):
            ins += list(q)
            aux |= int(w) << (8 + t)
        while len(ins) < 24:
            ins.append(ZERO)
        return Vec(tag, ins, aux)
    vecs = []
    for T in range(1, 7):
        for w in (0, 1):
            vecs.append(vec("maxcol:T%d:w%d" % (T, w), [((amx, amx, gmx, gmx), w)] * T))
            vecs.append(vec("maxcol:T%d:w%d:g1=0" % (T, w), [((amx, amx, gmx, lo), w)] * T))      # 4p - g1 at its largest
            vecs.append(vec("maxcol:T%d:w%d:a1=0" % (T, w), [((amx, lo, gmx, gmx), w)] * T))      # a0 - a1 + 8p at its largest
    ac, gc = operand_classes(rnd, 4 * P + 1, N_MAX, nrand=8), operand_classes(rnd, 2 * P, E_MAX, nrand=8)
    for i in range(90):
        T = 1 + i % 6
        vecs.append(vec("%s:%d" % (("random", "value")[i % 2], i), [((rnd.choice(ac)[1], rnd.choice(ac)[1], rnd.choice(gc)[1], rnd.choice(gc)[1]), rnd.randrange(2)) for _ in range(T)]))
    rnd.shuffle(vecs)
    return vecs


op("acc4", "kara", gen_acc4, legal_acc4, ref_acc4, peak_acc4)


# ------------------------------------------------------------------------------------------------------------------------------------
# xyzz_madd (ec.cuh): "XYZZ accumulator: X < 10p, Y < 6p, ZZ, ZZZ < 2p; affine inputs x, y < 4p"; limb classes of the lazy G1 form:
# "acc.x is N, acc.y / acc.zz / acc.zzz are E; x2 is E, y2 is E or U (negated)" (acc.y of a bucket's first point is N: FA::norm(y)).
#   P = x2 ZZ - X, R = y2 ZZZ - Y, PP = P^2, PPP = P PP, Q = X PP, X3 = R^2 - PPP - 2Q, Y3 = R (Q - X3) - Y PPP, ZZ3 = ZZ PP, ZZZ3 = ZZZ PPP
def madd_ref_fp(ins):
    X, Y, ZZ, ZZZ, x2, y2 = (val(l) % P for l in ins)
    m = lambda a, b: a * b * RINV % P
    Pd = (m(x2, ZZ) - X) % P
    if Pd == 0:
        return None
    Rr = (m(y2, ZZZ) - Y) % P
    PP = m(Pd, Pd)
    PPP = m(Pd, PP)
    Q = m(X, PP)
    X3 = (m(Rr, Rr) - PPP - 2 * Q) % P
    return X3, (m(Rr, (Q - X3) % P) - m(Y, PPP)) % P, m(ZZ, PP), m(ZZZ, PPP)


def gen_madd_g1(name):
    rnd = _rnd(name)
    cX, cY = operand_classes(rnd, 10 * P, N_MAX, nrand=8), operand_classes(rnd, 6 * P, N_MAX, nrand=8)
    cZ, cx = operand_classes(rnd, 2 * P, E_MAX, nrand=8), operand_classes(rnd, 4 * P, E_MAX, nrand=8)
    mx = [cX[0][1], cY[0][1], cZ[0][1], distinct_max(2 * P, E_MAX)[1], cx[0][1]]
    y2s = [("E", distinct_max(4 * P, E_MAX)[1]), ("U:S4", lazy_neg(4, ZERO)), ("U:S4-1", lazy_neg(4, exact(1))), ("U:rand", lazy_neg(4, exact(rnd.randrange(2 * P))))]
    vecs = [Vec("maxcol:y2=" + t, mx + [y]) for t, y in y2s]
    for i, cls in enumerate((cX, cY, cZ, cZ, cx)):
        for t, l in cls[1:]:
            ins = [l if j == i else rnd.choice(c)[1] for j, c in enumerate((cX, cY, cZ, cZ, cx))]
            y = rnd.choice(cx)[1]
            vecs.append(Vec("%s/%d" % (t, i), ins + [lazy_neg(4, y) if val(y) < 3 * P and rnd.randrange(2) else y]))
    # exceptional pairs: x2 ZZ == X (mod p), X = the product's residue + j p for every j below 10, ZZ at several classes
    for j in range(10):
        zz, x2 = rnd.choice(cZ)[1], rnd.choice(cx)[1]
        u = mont((x2, zz))
        if u + j * P < 10 * P:
            vecs.append(Vec("exc:+%dp" % j, [exact(u + j * P), rnd.choice(cY)[1], zz, rnd.choice(cZ)[1], x2, rnd.choice(cx)[1]]))
    vecs.append(Vec("exc:zero", [ZERO, cY[0][1], cZ[0][1], cZ[0][1], ZERO, cx[0][1]]))
    vecs.append(Vec("exc:zz=p", [exact(P), cY[0][1], exact(P), cZ[0][1], cx[0][1], cx[0][1]]))
    return vecs


def legal_madd_g1(v):
    X, Y, ZZ, ZZZ, x2, y2 = v.ins
    assert lowmax(X) <= N_MAX and val(X) < 10 * P and lowmax(Y) <= N_MAX and val(Y) < 6 * P
    assert all(lowmax(l) <= E_MAX and val(l) < 2 * P for l in (ZZ, ZZZ)) and lowmax(x2) <= E_MAX and val(x2) < 4 * P
    assert val(y2) <= 4 * P and all(x < E_MAX + SUB_LAZY_GROW for x in y2[:13])


def ref_madd(v, ncomp=1):
    if ncomp == 1:
        r = madd_ref_fp(v.ins)
    else:
        r = madd_ref_fp2(v.ins)
    if r is None:    # "Returns true without touching acc when the x-coordinates agree"
        return [Out(equal=l) for l in v.ins[:4 * ncomp]], 1
    outs = []
    for k, comp in enumerate(r):
        for c in (comp if ncomp == 2 else (comp,)):
            outs.append(Out(res=c, lo=0, hi=10 * P, limbs="N") if k == 0 else Out(res=c, **MUL_OUT))
    return outs, 0


def peak_madd_g1(v):
    X, Y, ZZ, ZZZ, x2, y2 = v.ins
    if madd_ref_fp(v.ins) is None:
        return 0
    pk = []

    def mm(*pairs):
        r, p = model_mul(*pairs)
        pk.append(p)
        return r
    t0 = model_sub(16, mm((x2, ZZ)), X, lazy=True)
    t2 = mm((t0, t0))
    t1 = model_sub(8, mm((y2, ZZZ)), Y, lazy=True)
    t0 = mm((t0, t2))
    mm((ZZ, t2))
    t2 = mm((X, t2))
    mm((ZZZ, t0))
    ny = model_sub(8, ZERO, Y, lazy=True)
    t3 = model_add(model_add(t0, t2, True), t2, True)
    X3 = model_norm(model_sub(8, mm((t1, t1)), t3, lazy=True, wide=True))
    t2 = model_sub(16, t2, X3, lazy=True)
    mm((t1, t2), (ny, t0))
    return max(pk)


op("madd_g1", "madd", gen_madd_g1, legal_madd_g1, ref_madd, peak_madd_g1)


def madd_ref_fp2(ins):
    X, Y, ZZ, ZZZ, x2, y2 = (f2(ins[2 * k], ins[2 * k + 1]) for k in range(6))
    m = lambda a, b: tuple(c * RINV % P for c in f2mul(a, b))
    sub = lambda a, b: ((a[0] - b[0]) % P, (a[1] - b[1]) % P)
    Pd = sub(m(x2, ZZ), X)
    if Pd == (0, 0):
        return None
    Rr = sub(m(y2, ZZZ), Y)
    PP = m(Pd, Pd)
    PPP = m(Pd, PP)
    Q = m(X, PP)
    X3 = sub(sub(m(Rr, Rr), PPP), ((2 * Q[0]) % P, (2 * Q[1]) % P))
    return X3, sub(m(Rr, sub(Q, X3)), m(Y, PPP)), m(ZZ, PP), m(ZZZ, PPP)


def gen_madd_g2(name):
    rnd = _rnd("madd_g2")
    cX, cY = fp2_classes(rnd, 10 * P, N_MAX, nrand=6), fp2_classes(rnd, 6 * P, N_MAX, nrand=6)
    cZ, cx = fp2_classes(rnd, 2 * P, E_MAX, nrand=6), fp2_classes(rnd, 4 * P, N_MAX, nrand=6)
    all_c = (cX, cY, cZ, cZ, cx, cx)
    vecs = [Vec("maxcol:all", [l for c in all_c for l in c[0][1:3]])]
    for i, cls in enumerate(all_c):
        for t, x0, x1 in cls[1:]:
            ins = []
            for j, c in enumerate(all_c):
                y = (t, x0, x1) if i == j else rnd.choice(c)
                ins += [y[1], y[2]]
            vecs.append(Vec("%s/%d" % (t, i), ins))
    for j in range(10):     # exceptional pairs: x2 ZZ == X in BOTH components (the verdict is pair-wide); one component alone is not
        zz, x2 = rnd.choice(cZ), rnd.choice(cx)
        u = tuple(c * RINV % P for c in f2mul(f2(x2[1], x2[2]), f2(zz[1], zz[2])))
        k0, k1 = j % 10, (3 * j + 1) % 10
        y, zzz, y2 = rnd.choice(cY), rnd.choice(cZ), rnd.choice(cx)
        rest = [y[1], y[2], zz[1], zz[2], zzz[1], zzz[2], x2[1], x2[2], y2[1], y2[2]]
        if u[0] + k0 * P < 10 * P and u[1] + k1 * P < 10 * P:
            vecs.append(Vec("exc:+%dp,+%dp" % (k0, k1), [exact(u[0] + k0 * P), exact(u[1] + k1 * P)] + rest))
            vecs.append(Vec("slow:c0 only", [exact(u[0] + k0 * P), exact((u[1] + 1) % P)] + rest))
            vecs.append(Vec("slow:c1 only", [exact((u[0] + 5) % P), exact(u[1] + k1 * P)] + rest))
    rnd.shuffle(vecs)
    return vecs


def legal_madd_g2(v):
    for k, (bound, low) in enumerate(((10, N_MAX), (6, N_MAX), (2, E_MAX), (2, E_MAX), (4, N_MAX), (4, N_MAX))):
        for l in v.ins[2 * k: 2 * k + 2]:
            assert lowmax(l) <= low and val(l) < bound * P


op("madd_g2", "madd", gen_madd_g2, legal_madd_g2, lambda v: ref_madd(v, 2))
# the same step with one lane per Fp2 value (ec::Fp2OpsInline, the field of k_accumulate<G2C>): has a host build, which pins the Fp2
# reference of the step without a GPU
op("madd_g2_lane", "madd", gen_madd_g2, legal_madd_g2, lambda v: ref_madd(v, 2))


# ------------------------------------------------------------------------------------------------------------------------------------
# Conversions to / from the reference's words (fp28.cuh).  The 12 words travel in limbs 0..11 of the slot.
#   fp_to_blst: "internal (any value < ~50p) -> blst Montgomery words, canonical": a limb vector of value V stands for V 2^-392, its words
#   are the integer V 2^-392 2^384 mod p, below p.
#   fp_from_blst: "blst Montgomery words (x*2^384 mod p)  ->  internal (x*2^392 mod p), N-form < 2p".  The comment speaks of words that ARE
#   x 2^384 mod p, i.e. below p; for words that are not below p (p, 2^384 - 1) it promises nothing, so only words below p are tested.
TO_BLST_BOUND = 50 * P


def words12(v):
    assert 0 <= v < 1 << 384
    return [(v >> (32 * k)) & 0xFFFFFFFF for k in range(12)] + [0, 0]


def val_words(l):
    return sum(int(x) << (32 * k) for k, x in enumerate(l[:12]))


def gen_from_blst(name):
    rnd = _rnd(name)
    vals = [0, 1, 2, P - 2, (1 << 384) % P, (1 << 392) % P, 1 << 380, (1 << 380) - 1, 0xFFFFFFFF, 1 << 32, P >> 1]
    vals += [1 << (28 * k) for k in range(1, 14)] + [(1 << (32 * k)) - 1 for k in range(1, 12)]      # limb and word seams of the re-limbing
    vals += [((1 << 384) - 1) // 3 % P, int("a5" * 48, 16) % P, int("5a" * 48, 16) % P]
    vecs = [Vec("maxcol:p-1", [words12(P - 1)])]             # the top of the contract: the largest words below p
    vecs += [Vec("value:%d" % i, [words12(v)]) for i, v in enumerate(vals)]
    vecs += [Vec("random:%d" % i, [words12(rnd.randrange(P))]) for i in range(40)]
    return vecs


def legal_from_blst(v):
    assert val_words(v.ins[0]) < P and v.ins[0][12:] == [0, 0] and all(0 <= x < 1 << 32 for x in v.ins[0])


op("fp_from_blst", "conv", gen_from_blst, legal_from_blst, lambda v: ([Out(res=val_words(v.ins[0]) << 8, lo=0, hi=2 * P, limbs="N")], None))
op("fp_to_blst", "conv", lambda name: gen_one(TO_BLST_BOUND, N_MAX, name, nrand=40), lambda v: legal_nform(TO_BLST_BOUND, v),
   lambda v: ([Out(equal=words12(val(v.ins[0]) * pow(1 << 8, -1, P) % P))], None))


# ------------------------------------------------------------------------------------------------------------------------------------
# One step of the G2 point walk of k_miller_lines2 (pairing_kernels.cuh coop_line_dbl / coop_line_add, "the formulas of
# pairing::Tower::line_dbl / line_add"), two lanes per element.  Operands: T = (X, Y, Z) over Fp2, then (-xP | yP), then (xQ, yQ) for the
# addition.  A limb vector of value V stands for the field element V 2^-392; the reference is the formula of the comment over Fp2 in
# Python integers, the expected residue is result 2^392.  pairing.cuh line_dbl:
#   "B = Y^2, C = Z^2, E = b3 C = 3b' Z^2, H = (Y + Z)^2 - B - C = 2YZ:  X3 = 2 XY (B - 3E),  Y3 = (B + 3E)^2 - 12 E^2,  Z3 = 4 H B ...
#    The line is (B - E) + (-3 X^2 xP) v + (H yP) v w.  T <= 6p in, < 4p out."   c0 "< 6p", T.x "< 4p", T.z, T.y "< 2p"
# line_add: "N = Y - yQ Z (< 10p: so T.y <= 6p as in line_dbl), D = X - xQ Z, c0 = N xQ - D yQ (< 6p), c1 = N (-xP), c4 = D yP", then
#   T <- T + Q by ec::proj_add "complete (RCB16 Alg. 7)": with b3 = 12 (1 + u) and Z2 = 1
#     X3 = (X1Y2 + X2Y1)(Y1Y2 - b3 Z1) - b3 (Y1 + Y2Z1)(X1 + X2Z1),  Y3 = (Y1Y2 - b3 Z1)(Y1Y2 + b3 Z1) + 3 X1X2 b3 (X1 + X2Z1),
#     Z3 = (Y1Y2 + b3 Z1)(Y1 + Y2Z1) + 3 X1X2 (X1Y2 + X2Y1);
#   every output of CoopF2's proj_add is mul2add = "fp_add(mul(a, b), mul(c, d))", the sum of two products of < 2p: N-form, < 4p.
#   T = Q: N = D = 0, the line is zero, and the complete addition returns 2Q (Z3 != 0); T = -Q: D = 0, c4 = 0, and it returns the point
#   at infinity (0 : Y3 : 0), Y3 != 0.  Both are checked against the integer formula like every other vector (and, for a Q on the curve,
#   against the affine doubling) — gen_line marks them "exc".
# P as the kernel gets it: -xP = fp_neg<4>(x) of x = fp_from_blst(..) < 2p: N-form, value in (2p, 4p]; yP, xQ, yQ = fp_from_blst(..):
#   multiplier outputs, exact limbs, < 2p.
# aux bit 0 = the LineSink's `inf` (P or Q at infinity): the stored line must be exactly (CoopF2::one(), 0, 0); T is walked all the same.
B3 = (12, 12)
LINE_T = 6 * P + 1      # "T <= 6p in"


def _elem(l):
    return val(l) * RINV % P


def _e2(l0, l1):
    return (_elem(l0), _elem(l1))


def f2add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def f2sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def f2k(k, a):
    return (k * a[0] % P, k * a[1] % P)


def line_dbl_formula(X, Y, Z, nx, yp):
    """(c0, c1, c4, X3, Y3, Z3) as field elements"""
    B, Cc = f2mul(Y, Y), f2mul(Z, Z)
    H = f2k(2, f2mul(Y, Z))
    E = f2mul(B3, Cc)
    c0, c4, c1 = f2sub(B, E), f2k(yp, H), f2k(3 * nx, f2mul(X, X))
    E3 = f2k(3, E)
    X3 = f2k(2, f2mul(f2mul(X, Y), f2sub(B, E3)))
    Z3 = f2k(4, f2mul(H, B))
    s = f2add(B, E3)
    Y3 = f2sub(f2mul(s, s), f2k(12, f2mul(E, E)))
    return c0, c1, c4, X3, Y3, Z3


def line_add_formula(X, Y, Z, nx, yp, xq, yq):
    N, D = f2sub(Y, f2mul(yq, Z)), f2sub(X, f2mul(xq, Z))
    c0, c1, c4 = f2sub(f2mul(N, xq), f2mul(D, yq)), f2k(nx, N), f2k(yp, D)
    xx, yy, bz = f2mul(X, xq), f2mul(Y, yq), f2mul(B3, Z)
    xy = f2add(f2mul(X, yq), f2mul(xq, Y))
    yz, xz = f2add(Y, f2mul(yq, Z)), f2add(X, f2mul(xq, Z))
    lo, hi = f2sub(yy, bz), f2add(yy, bz)
    X3 = f2sub(f2mul(xy, lo), f2mul(f2mul(B3, yz), xz))
    Y3 = f2add(f2mul(lo, hi), f2mul(f2k(3, xx), f2mul(B3, xz)))
    Z3 = f2add(f2mul(hi, yz), f2mul(f2k(3, xx), xy))
    return c0, c1, c4, X3, Y3, Z3


def _line_keep(tag):
    head = tag.split(":")[0]
    return head in ("maxcol", "value", "random") or tag in ("spell:0", "spell:1", "spell:5", "slow:0", "slow:3", "pattern:alt0", "pattern:alt1", "pattern:hot0",
                                                            "pattern:hot12", "pattern:hot13")


def _mont_exact(x):
    return exact(x * R % P)


def gen_line(add, name):
    rnd = _rnd(name)
    cls = [[c for c in operand_classes(rnd, LINE_T, N_MAX, nrand=4) if _line_keep(c[0])] for _ in range(6)]      # X0 X1 Y0 Y1 Z0 Z1
    cls.append([c for c in operand_classes(rnd, 4 * P + 1, N_MAX, nrand=4, lo_value=2 * P + 1) if _line_keep(c[0])])   # -xP
    for _ in range(5 if add else 1):                                                                               # yP, xQ (2), yQ (2)
        cls.append([c for c in operand_classes(rnd, 2 * P, E_MAX, nrand=4) if _line_keep(c[0])])
    nop = len(cls)
    tmax = [l for pair in (distinct_max(LINE_T), distinct_max(LINE_T), distinct_max(LINE_T)) for l in pair]
    pq_max = [maxlow(4 * P + 1)] + [maxlow(2 * P, E_MAX)] + ([l for pair in (distinct_max(2 * P, E_MAX), distinct_max(2 * P, E_MAX)) for l in pair] if add else [])
    pq_min = [exact(2 * P + 1)] + [ZERO] * (nop - 7)
    vecs = [Vec("maxcol:all", tmax + pq_max), Vec("maxcol:T/min", tmax + pq_min), Vec("maxcol:PQ/min", [ZERO] * 6 + pq_max)]
    for i in range(nop):
        for t, l in cls[i]:
            vecs.append(Vec("%s/%d" % (t, i), [l if j == i else rnd.choice(cls[j])[1] for j in range(nop)]))
    # structural vectors: a coordinate of T zero in both components (every pair of spellings of zero), xP = 0 (-xP = 4p or 3p), yP = 0
    zs = [ZERO, exact(P), exact(2 * P), exact(6 * P)]
    rand = lambda: [rnd.choice(cls[j])[1] for j in range(nop)]
    for coord, cname in enumerate("XYZ"):
        for i, (z0, z1) in enumerate(((zs[0], zs[0]), (zs[1], zs[0]), (zs[0], zs[2]), (zs[3], zs[1]))):
            ins = rand()
            ins[2 * coord], ins[2 * coord + 1] = z0, z1
            vecs.append(Vec("zero:%s=0:%d" % (cname, i), ins))
    for i, z in enumerate((exact(4 * P), exact(3 * P))):
        ins = rand()
        ins[6] = z
        vecs.append(Vec("zero:xP=0:%d" % i, ins))
    for i, z in enumerate((ZERO, exact(P))):
        ins = rand()
        ins[7] = z
        vecs.append(Vec("zero:yP=0:%d" % i, ins))
    ins = rand()
    ins[0:6] = [ZERO, ZERO, C["ONE"], ZERO, ZERO, ZERO]
    vecs.append(Vec("zero:T=infinity(0:1:0)", ins))
    if add:   # T = Q and T = -Q, for Q on the twist (the G2 generator and a multiple) and T = (s xQ, +-s yQ, s) in several scalings
        from oracle import bls12_381 as o

        for qi, Q in enumerate((o.G2_GEN, o.scalar_mul(o.F2, o.G2_GEN, 0xABCDEF0123456789))):
            for si, s in enumerate(((1, 0), (5, 0), (rnd.randrange(P), rnd.randrange(P)))):
                for sign in (1, -1):
                    tx, ty = f2mul(Q[0], s), f2k(sign, f2mul(Q[1], s))
                    ins = rand()
                    ins[0:6] = [_mont_exact(c) for c in (tx[0], tx[1], ty[0], ty[1], s[0], s[1])]
                    ins[8:12] = [_mont_exact(c) for c in (Q[0][0], Q[0][1], Q[1][0], Q[1][1])]
                    vecs.append(Vec("exc:T=%sQ:%d:%d" % ("+" if sign > 0 else "-", qi, si), ins))
    # the same step with the sink's `inf` set: every eighth vector again
    vecs += [Vec("inf:" + v.tag, v.ins, 1) for v in vecs[::8]]
    rnd.shuffle(vecs)
    return vecs


def legal_line(add, v):
    assert len(v.ins) == (12 if add else 8) and v.aux in (0, 1)
    for l in v.ins[:6]:
        assert lowmax(l) <= N_MAX and val(l) <= 6 * P                   # "T <= 6p in", N-form
    assert lowmax(v.ins[6]) <= N_MAX and 2 * P < val(v.ins[6]) <= 4 * P  # fp_neg<4> of a value below 2p
    for l in v.ins[7:]:
        assert lowmax(l) <= E_MAX and val(l) < 2 * P                    # fp_from_blst: a multiplier output


def line_elems(v):
    X, Y, Z = _e2(*v.ins[0:2]), _e2(*v.ins[2:4]), _e2(*v.ins[4:6])
    return [X, Y, Z, _elem(v.ins[6]), _elem(v.ins[7])] + ([_e2(*v.ins[8:10]), _e2(*v.ins[10:12])] if len(v.ins) == 12 else [])


def ref_line(add, v):
    r = (line_add_formula if add else line_dbl_formula)(*line_elems(v))
    outs = []
    tb = (4, 4, 4) if add else (4, 2, 2)      # the new T: line_dbl "T.x < 4p, T.z < 2p, T.y < 2p"; proj_add over CoopF2: sums of two products
    for k, c in enumerate(r):
        hi = (6, 2, 2)[k] if k < 3 else tb[k - 3]
        for comp in (0, 1):
            if v.aux & 1 and k < 3:
                outs.append(Out(equal=C["ONE"] if (k, comp) == (0, 0) else ZERO))
            else:
                outs.append(Out(res=c[comp] * R, lo=0, hi=hi * P, limbs="N"))
    if "exc:T=+" in v.tag:                                                  # T = Q: the zero line, and 2Q (the affine doubling's point)
        from oracle import bls12_381 as o

        q2 = o.scalar_mul(o.F2, tuple(line_elems(v)[5:7]), 2)
        assert r[0] == r[1] == r[2] == (0, 0) and r[5] != (0, 0)
        assert r[3] == f2mul(q2[0], r[5]) and r[4] == f2mul(q2[1], r[5])
    if "exc:T=-" in v.tag:                                                  # T = -Q: a vertical line, and infinity
        assert r[2] == (0, 0) and r[3] == r[5] == (0, 0) and r[4] != (0, 0)
    return outs, None


for _add, _n in ((False, "line_dbl"), (True, "line_add")):
    op(_n, "line", (lambda name, a=_add: gen_line(a, name)), (lambda v, a=_add: legal_line(a, v)), (lambda v, a=_add: ref_line(a, v)))

MODELS = {"kara": lambda v: model_kara(v)[:2], "kara_pre": lambda v: model_kara(v, True)[:2], "acc4": lambda v: model_acc4(v)[:2]}

FAMILIES = sorted({d["family"] for d in OPS.values()})
_CACHE = {}


def vectors(name):
    """the legal vectors of op `name` (generated once per process, never modified)"""
    if name not in _CACHE:
        vecs = OPS[name]["gen"](name)
        assert 16 <= len(vecs) <= 4096, (name, len(vecs))
        for v in vecs:
            try:
                OPS[name]["legal"](v)
            except AssertionError as e:
                raise AssertionError("%s [%s]: vector outside the op's documented input contract: %s" % (name, v.tag, e))
        _CACHE[name] = vecs
    return _CACHE[name]


def pack(vecs, in_slots):
    """vectors -> the hook's operand bytes: 16-word slots, word 15 of an element's first slot = aux"""
    import struct

    out = bytearray()
    for v in vecs:
        assert len(v.ins) == in_slots, (len(v.ins), in_slots)
        for k, l in enumerate(v.ins):
            out += struct.pack("<16I", *l, 0, v.aux if k == 0 else 0)
    return bytes(out)


def unpack(data, out_slots):
    """result bytes -> per element ([14 limbs] per result slot, verdict)"""
    import struct

    words = struct.unpack("<%dI" % (len(data) // 4), data)
    res = []
    for e in range(len(words) // (16 * out_slots)):
        base = e * 16 * out_slots
        res.append(([list(words[base + 16 * k: base + 16 * k + 14]) for k in range(out_slots)], words[base + 15]))
    return res


def check(name, results):
    """assert every result of op `name` (unpack()ed, in the order of vectors(name)) against the reference and the output contract;
    returns the tags of the failing vectors' classes instead when collect is asked for by check_collect"""
    bad = check_collect(name, results)
    assert not bad, "%s: %d of %d vectors fail, first: %s" % (name, len(bad), len(results), bad[0][1])


def check_collect(name, results):
    vecs = vectors(name)
    assert len(results) == len(vecs)
    bad = []
    for v, (slots, flag) in zip(vecs, results):
        try:
            outs, want_flag = OPS[name]["ref"](v)
            assert len(outs) == len(slots), "result slots"
            for k, (l, w) in enumerate(zip(slots, outs)):
                check_out(name, v, k, l, w)
            assert flag == (want_flag or 0), "%s [%s]: verdict %d, expected %d" % (name, v.tag, flag, want_flag or 0)
        except AssertionError as e:
            bad.append((v.tag, str(e)))
    return bad


def peak_fraction(name):
    """largest |column| the vectors of `name` reach in the 64-bit accumulators, as a fraction of 2^64 (unsigned) or 2^63 (signed Karatsuba
    columns); None for ops without column arithmetic of their own"""
    pk = OPS[name]["peak"]
    if pk is None:
        return None
    limit = 1 << (63 if name in ("kara", "kara_pre") else 64)
    return max(pk(v) for v in vectors(name)) / limit


# ------------------------------------------------------------------------------------------------------------------------------------
_HOST = []


def host_lib():
    """the host build (g++) of the device headers with the raw-limb entry h28_field_op (tests/host/fp28_host_check.cpp)"""
    if not _HOST:
        import ctypes
        import subprocess

        here = os.path.join(ROOT, "tests", "host")
        so = os.path.join(here, "libfp28_field.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(here, "fp28_host_check.cpp")])
        L = ctypes.CDLL(so)
        L.h28_field_op.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
        L.h28_field_op_info.argtypes = [ctypes.c_int] + [ctypes.POINTER(ctypes.c_int)] * 3
        L.h28_field_op_info.restype = ctypes.c_char_p
        _HOST.append(L)
    return _HOST[0]


def host_ops():
    """[(name, operand slots, result slots, kind)] of the op table, index = op number (kind 0: has a host build)"""
    import ctypes

    L, ops = host_lib(), []
    a, b, k = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    while True:
        name = L.h28_field_op_info(len(ops), ctypes.byref(a), ctypes.byref(b), ctypes.byref(k))
        if not name:
            return ops
        ops.append((name.decode(), a.value, b.value, k.value))


_HOST_RESULTS = {}


def host_run(name):
    """raw result bytes of op `name` on its vectors from the host build (computed once)"""
    if name not in _HOST_RESULTS:
        import ctypes

        ops = host_ops()
        idx = [o[0] for o in ops].index(name)
        _, nin, nout, kind = ops[idx]
        assert kind == 0, name + " has no host build"
        vecs = vectors(name)
        out = ctypes.create_string_buffer(64 * nout * len(vecs))
        assert host_lib().h28_field_op(idx, pack(vecs, nin), len(vecs), out) == 0
        _HOST_RESULTS[name] = out.raw
    return _HOST_RESULTS[name]
