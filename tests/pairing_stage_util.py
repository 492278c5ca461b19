"""Constructed inputs, integer references and checkers for the production kernels of the pairing row, one stage at a time
(mi_test_pairing_stage, csrc/test_hooks.h): k_miller_accumulate on whole line buffers, k_fp12_prod on one tree level, k_fp12_to_raw.
The line steps (coop_line_dbl / coop_line_add) and the conversions are ops of the field table: tests/field_vectors_util.py.

Shared by tests/test_pairing_stage_cpu.py (vectors legal, reference == host build of the generic tower, layout round trip) and
tests/test_gpu_pairing_stage.py (the device).  As in field_vectors_util: every input is asserted against the contract QUOTED from the
comment of the code under test before it is used; a limb vector of value V stands for the field element V 2^-392 mod p, the reference is
the plain formula over Fp2 / Fp12 in Python integers (oracle/pairing.py's flat Fp12 = Fp2[w]/(w^6 - xi)), the expected device residue is
result 2^392 mod p, compared exactly; the output contract of the comment is checked on the returned limbs.

pairing_kernels.cuh, above KaraCols (the contract of k_miller_accumulate's line product):
    "Operand bounds: a' <= (12p, 8p) in N-form, g <= 6p in N-form (a line's c0; exact coefficients are < 2p) ... The contract is the
     operand bounds AND sum a1' g1 <= 144 p^2"
  a' comes from the five-value record of f ("f exact (< 2p per component): s < 4p, d < 6p, d + s < 10p"): a1' < 4p whatever f is, so a
  line is legal when every component is N-form, c0 <= 6p, c1, c4 <= 2p (pairing.cuh mul_by_014: "c0 <= 6p, c1, c4 <= 2p") and
  4p (c0.c1 + c1.c1 + c4.c1) <= 144 p^2.  Output: "every output is < 2p", stored in tower slot c_{k&1}.c_{k>>1}.
pairing_kernels.cuh fp2_acc_term4 (the contract of k_fp12_prod's product in[2g] * in[2g+1]):
    "a <= 4p, g exact (< 2p) ... six terms per reduction"; the result is fp_mont_reduce's: "Returns exact limbs, < 2p".
k_fp12_to_raw is fp_to_blst per coefficient: "internal (any value < ~50p) -> blst Montgomery words, canonical".
"""
import os
import random
import struct
import time

import tests.field_vectors_util as fv
from tests.field_vectors_util import C, E_MAX, N_MAX, NL, P, R, RINV, ZERO, exact, lowmax, maxlow, rand_nform, val

SEED = 0x9A121
MILLER_LINES = 68
Z_ABS = 0xD201000000010000
FP12_SLOTS = 12                     # 16-word slots of a device-form Fp12, order c0.c0.c0, c0.c0.c1, c0.c1.c0, ... as blst_fp12
TOWER_OF_FLAT = [(k & 1) * 3 + (k >> 1) for k in range(6)]      # flat w^k -> tower slot c_{k&1}.c_{k>>1} (an Fp2 = two 16-word slots)
ONE = C["ONE"]


def _rnd(name):
    return random.Random("%x:%s" % (SEED, name))


# ------------------------------------------------------------------------------------------------------------------------------------
# layout of the line buffer: "[block of `blk` pairs][line][pair in block][3 Fp2 slots of 32 words]", blk = 10 m
def line_base_words(pair, blk):
    """word offset of line 0 of `pair`; line l is l * blk * 96 words on (pairing_kernels.cuh line_base_words)"""
    b, i = divmod(pair, blk)
    return (b * MILLER_LINES * blk + i) * 96


def line_buffer_words(n, m):
    blk = 10 * m
    return (n + blk - 1) // blk * blk * MILLER_LINES * 96


def coeff_words(pair, line, slot, comp, blk):
    return line_base_words(pair, blk) + line * blk * 96 + 32 * slot + 16 * comp


def pack_lines(lines, n, m, fill=0xFFFFFFFF):
    """lines[pair][line] = (c0, c1, c4), each ((14 limbs), (14 limbs)) -> the buffer's bytes.  The slots of the pairs beyond n in the
    last block are filled with `fill`: production leaves them unwritten, the kernel must not read them."""
    blk = 10 * m
    words = line_buffer_words(n, m)
    buf = bytearray(struct.pack("<I", fill) * words)
    for pair in range(n):
        for line in range(MILLER_LINES):
            for slot in range(3):
                for comp in (0, 1):
                    struct.pack_into("<16I", buf, 4 * coeff_words(pair, line, slot, comp, blk), *lines[pair][line][slot][comp], 0, 0)
    return bytes(buf)


def unpack_lines(data, n, m):
    blk = 10 * m
    out = []
    for pair in range(n):
        out.append([tuple(tuple(list(struct.unpack_from("<14I", data, 4 * coeff_words(pair, line, slot, comp, blk))) for comp in (0, 1))
                          for slot in range(3)) for line in range(MILLER_LINES)])
    return out


def pack_fp12(values):
    """values[i] = 12 limb vectors in tower (blst_fp12) order -> bytes"""
    return b"".join(struct.pack("<16I", *l, 0, 0) for v in values for l in v)


def unpack_fp12(data):
    n = len(data) // (64 * FP12_SLOTS)
    return [[list(struct.unpack_from("<14I", data, 64 * (FP12_SLOTS * i + s))) for s in range(FP12_SLOTS)] for i in range(n)]


# ------------------------------------------------------------------------------------------------------------------------------------
# flat Fp12 over field elements (Python integers mod p)
def _pr():
    from oracle import pairing

    return pairing


def elem(l):
    return val(l) * RINV % P


def flat_of_limbs(v):
    """12 limb vectors in tower order -> six Fp2 coefficients of w^0 .. w^5 as field elements"""
    return [(elem(v[2 * TOWER_OF_FLAT[k]]), elem(v[2 * TOWER_OF_FLAT[k] + 1])) for k in range(6)]


def residues_of_flat(f):
    """expected device residues (x 2^392 mod p) of a flat Fp12, per 16-word slot in tower order"""
    out = [None] * FP12_SLOTS
    for k in range(6):
        out[2 * TOWER_OF_FLAT[k]], out[2 * TOWER_OF_FLAT[k] + 1] = f[k][0] * R % P, f[k][1] * R % P
    return out


def line_flat(line):
    """a line (c0, c1, c4) -> the sparse flat element c0 + c1 w^2 + c4 w^3 ("A line is sparse (w^0, w^2, w^3)")"""
    c0, c1, c4 = ((elem(c[0]), elem(c[1])) for c in line)
    return [c0, (0, 0), c1, c4, (0, 0), (0, 0)]


def ref_accumulate(lines, n, m):
    """out[g] for g < ceil(n / m): f = 1; per bit of |z| from 62 down f <- f^2, then f <- f l for each live pair's line (again for the
    addition line where the bit is set); conjugated (odd coefficients negated).  Flat Fp12 values as field elements."""
    pr = _pr()
    out = []
    for g in range((n + m - 1) // m):
        pairs = range(g * m, min(n, g * m + m))
        f = list(pr.FP12_ONE)
        line = 0
        for b in range(62, -1, -1):
            f = pr.fp12_mul(f, f)
            for _ in range(2 if (Z_ABS >> b) & 1 else 1):
                for pair in pairs:
                    f = pr.fp12_mul(line_flat(lines[pair][line]), f)
                line += 1
        assert line == MILLER_LINES
        out.append([c if k % 2 == 0 else ((-c[0]) % P, (-c[1]) % P) for k, c in enumerate(f)])
    return out


def check_fp12(where, limbs, want_flat, hi=2 * P, exact_limbs=False):
    """12 returned limb vectors against the expected flat value: residues exactly, every coefficient below `hi`, N-form (or exact) limbs"""
    want = residues_of_flat(want_flat)
    for s in range(FP12_SLOTS):
        v = val(limbs[s])
        assert v % P == want[s], "%s slot %d: wrong residue" % (where, s)
        assert v < hi, "%s slot %d: value %.4f p not below %d p" % (where, s, v / P, hi // P)
        assert lowmax(limbs[s]) <= (E_MAX if exact_limbs else N_MAX), "%s slot %d: limbs outside the promised form" % (where, s)


# ------------------------------------------------------------------------------------------------------------------------------------
# k_miller_accumulate: line buffers
ACC_SHAPES = sorted({(m, n) for m in (1, 2, 7, 8) for n in (1, m, m + 1, 10 * m, 10 * m + 1)})
PAIR_CLASSES = ["maxcol", "random", "inf", "c0zero", "c14zero", "pz", "random", "maxcol"]
ZERO_LINE = 40        # the all-zero line of the "zero" accumulator sits in the middle of the loop


def legal_line(line):
    c0, c1, c4 = line
    for c, bound in ((c0, 6 * P), (c1, 2 * P), (c4, 2 * P)):
        for l in c:
            assert lowmax(l) <= N_MAX and l[NL - 1] < 1 << 24 and val(l) <= bound, "g <= 6p in N-form (c0), c1, c4 <= 2p"
    assert 4 * P * (val(c0[1]) + val(c1[1]) + val(c4[1])) <= 144 * P * P, "sum a1' g1 <= 144 p^2"


def _spell0(rnd, bound):
    """a representation of zero: k p, k p <= bound"""
    return exact(rnd.randrange(bound // P + 1) * P)


def make_line(rnd, cls):
    top = fv.distinct_max(6 * P + 1)
    e2 = lambda: (exact(rnd.randrange(2 * P)), exact(rnd.randrange(2 * P)))
    n6 = lambda: (rand_nform(rnd, 6 * P + 1), rand_nform(rnd, 6 * P + 1))
    if cls == "maxcol":       # every c0 at the top of 6p with maximal N-form limbs, c1 and c4 at 2p - 1
        return ((top[0], top[1]), (exact(2 * P - 1), exact(2 * P - 1)), (exact(2 * P - 1), exact(2 * P - 1)))
    if cls == "inf":          # what the LineSink stores for a pair with P or Q at infinity: (CoopF2::one(), 0, 0)
        return ((ONE, ZERO), (ZERO, ZERO), (ZERO, ZERO))
    if cls == "c0zero":
        return ((_spell0(rnd, 6 * P), _spell0(rnd, 6 * P)), e2(), e2())
    if cls == "c14zero":
        return (n6(), (_spell0(rnd, 2 * P), _spell0(rnd, 2 * P)), (_spell0(rnd, 2 * P), _spell0(rnd, 2 * P)))
    if cls == "pz":           # coefficients that are p or 2p (zero, spelled both ways) next to live ones; never the whole line
        pz = lambda: exact(rnd.choice((P, 2 * P)))
        pick = rnd.randrange(1, 63)       # which of the six components are p / 2p: at least one, not all
        comps = [pz() if (pick >> i) & 1 else (rand_nform(rnd, 6 * P + 1) if i < 2 else exact(rnd.randrange(2 * P))) for i in range(6)]
        return ((comps[0], comps[1]), (comps[2], comps[3]), (comps[4], comps[5]))
    if cls == "zero":         # the all-zero line, in mixed spellings
        return ((_spell0(rnd, 6 * P), ZERO), (exact(P), _spell0(rnd, 2 * P)), (ZERO, exact(2 * P)))
    assert cls == "random"
    return (n6(), e2(), e2())


def shape_plan(m, n):
    """the class of every pair of the shape (m, n), and the pair whose line ZERO_LINE is all zero (or None)"""
    if n == m and m > 1:
        classes = ["maxcol"] * n                       # a whole accumulator of lines at the corner
    elif n == m + 1 and m > 2:
        classes = ["random"] * n
    else:
        classes = [PAIR_CLASSES[(i + m) % len(PAIR_CLASSES)] for i in range(n)]
    if n >= 10 * m and m > 1:
        # infinity pairs in the first, a middle and the last slot of a shared accumulator (groups 0, 1, 2), a whole group of them (group 5)
        classes[0] = classes[m + m // 2] = classes[3 * m - 1] = "inf"
        for i in range(5 * m, 6 * m):
            classes[i] = "inf"
    zero_pair = 3 * m + m // 2 if n >= 10 * m else None    # group 3: f is zero from ZERO_LINE on
    if n == 10 * m + 1:
        classes[n - 1] = "maxcol"                      # the lone pair of the second wave, shadowed by nine idle groups
    return classes, zero_pair


_ACC = {}


def acc_case(m, n):
    """(lines, packed bytes, classes, zero_pair) of the shape, generated once and never modified; every line asserted legal"""
    if (m, n) not in _ACC:
        rnd = _rnd("acc:%d:%d" % (m, n))
        classes, zero_pair = shape_plan(m, n)
        lines = []
        for pair in range(n):
            per = [make_line(rnd, classes[pair]) for _ in range(MILLER_LINES)]
            if pair == zero_pair:
                per[ZERO_LINE] = make_line(rnd, "zero")
            for ln in per:
                legal_line(ln)
            lines.append(per)
        _ACC[(m, n)] = (lines, pack_lines(lines, n, m), classes, zero_pair)
    return _ACC[(m, n)]


_ACC_REF = {}


def acc_reference(m, n):
    if (m, n) not in _ACC_REF:
        _ACC_REF[(m, n)] = ref_accumulate(acc_case(m, n)[0], n, m)
    return _ACC_REF[(m, n)]


def check_accumulate(m, n, out_bytes):
    got, want = unpack_fp12(out_bytes), acc_reference(m, n)
    assert len(got) == len(want) == (n + m - 1) // m
    _, _, _, zero_pair = acc_case(m, n)
    for g, (limbs, flat) in enumerate(zip(got, want)):
        check_fp12("accumulate m=%d n=%d group %d" % (m, n, g), limbs, flat)        # "every output is < 2p"
        if zero_pair is not None and g == zero_pair // m:
            assert all(c == (0, 0) for c in flat)      # after the all-zero line f is zero and stays a representation of zero
        else:
            assert any(c != (0, 0) for c in flat)


# ------------------------------------------------------------------------------------------------------------------------------------
# k_fp12_prod: one tree level
PROD_SIZES = [1, 2, 3, 19, 20, 21, 41]
W3_SLOT = 2 * TOWER_OF_FLAT[3]


def fp12_operand(rnd, cls, role):
    """12 limb vectors; role 'a' = the running product (even index: "a <= 4p", N-form), 'g' = the factor ("g exact (< 2p)")"""
    if role == "a":
        one_c = lambda: rand_nform(rnd, 4 * P + 1)
        top = fv.distinct_max(4 * P + 1)
    else:
        one_c = lambda: exact(rnd.randrange(2 * P))
        top = fv.distinct_max(2 * P, E_MAX)
    if cls == "zero0":
        return [ZERO] * 12
    if cls == "zerop":
        return [exact(P)] * 12
    if cls == "zeromix":
        return [exact(P) if (i * 5 + 1) % 3 else ZERO for i in range(12)]
    if cls == "one":
        return [ONE] + [ZERO] * 11
    if cls == "onep":         # one with every zero coefficient spelled p
        return [ONE] + [exact(P)] * 11
    if cls == "p-1":
        return [exact(P - 1)] * 12
    if cls == "2p-1":
        return [exact(2 * P - 1)] * 12
    if cls == "w0":           # sparse: only w^0
        return [one_c(), one_c()] + [ZERO] * 10
    if cls == "w3":           # sparse: only w^3 (tower slot c1.c1)
        return [one_c() if s in (W3_SLOT, W3_SLOT + 1) else ZERO for s in range(12)]
    if cls == "maxcol":
        return [top[s & 1] for s in range(12)]
    assert cls == "random"
    return [one_c() for _ in range(12)]


PROD_CLASSES = ["random", "zero0", "one", "p-1", "2p-1", "w0", "w3", "zerop", "maxcol", "zeromix", "onep"]


def legal_prod_operand(v, role):
    for l in v:
        if role == "a":
            assert lowmax(l) <= N_MAX and l[NL - 1] < 1 << 24 and val(l) <= 4 * P, "a <= 4p"
        else:
            assert lowmax(l) <= E_MAX and val(l) < 2 * P, "g exact (< 2p)"


_PROD = {}


def prod_case(n):
    """n device-form Fp12 values: the classes of the even (running product) and odd (factor) positions walk PROD_CLASSES at different
    strides, so every class meets several others; asserted legal; generated once"""
    if n not in _PROD:
        rnd = _rnd("prod:%d" % n)
        vals = []
        for i in range(n):
            role = "g" if i & 1 else "a"
            k = len(PROD_CLASSES)
            cls = PROD_CLASSES[((i // 2) * 4 + 1 + n) % k] if i & 1 else PROD_CLASSES[(i // 2 + n) % k]
            v = fp12_operand(rnd, cls, role)
            legal_prod_operand(v, role)
            vals.append(v)
        _PROD[n] = vals
    return _PROD[n]


def ref_prod(vals):
    pr = _pr()
    return [pr.fp12_mul(flat_of_limbs(vals[2 * g]), flat_of_limbs(vals[2 * g + 1])) for g in range(len(vals) // 2)]


def check_prod(n, out_bytes):
    vals, got = prod_case(n), unpack_fp12(out_bytes)
    want = ref_prod(vals)
    assert len(got) == (n + 1) // 2
    for g, flat in enumerate(want):
        check_fp12("prod n=%d group %d" % (n, g), got[g], flat, exact_limbs=True)     # fp_mont_reduce: "Returns exact limbs, < 2p"
    if n & 1:                 # "a group that is out of elements ... discards the result": the unpaired last value comes back limb for limb
        assert got[-1] == vals[-1], "prod n=%d: the unpaired last value was changed" % n


# ------------------------------------------------------------------------------------------------------------------------------------
# k_fp12_to_raw: device form -> blst_fp12 words, canonical
TO_RAW_N = 64


def to_raw_case():
    """64 Fp12 values = 768 coefficients from the classes of fp_to_blst's contract ("any value < ~50p", N-form): 0, 1,
    p - 1, p, p + 1, 2p - 1, random below 2p first, then every class up to 50p"""
    if "raw" not in _PROD:
        rnd = _rnd("to_raw")
        pool = [exact(v) for v in (0, 1, P - 1, P, P + 1, 2 * P - 1)] + [rand_nform(rnd, 2 * P) for _ in range(66)]
        pool += [l for _, l in fv.operand_classes(rnd, fv.TO_BLST_BOUND, N_MAX, nrand=40)]
        while len(pool) < 12 * TO_RAW_N:
            pool.append(rand_nform(rnd, rnd.choice((2 * P, 4 * P, fv.TO_BLST_BOUND))))
        pool = pool[:12 * TO_RAW_N]
        for l in pool:
            assert lowmax(l) <= N_MAX and val(l) < fv.TO_BLST_BOUND
        _PROD["raw"] = [pool[12 * i: 12 * i + 12] for i in range(TO_RAW_N)]
    return _PROD["raw"]


def check_to_raw(vals, out_bytes):
    assert len(out_bytes) == 576 * len(vals)
    inv8 = pow(1 << 8, -1, P)
    for i, v in enumerate(vals):
        for s in range(12):
            got = int.from_bytes(out_bytes[576 * i + 48 * s: 576 * i + 48 * s + 48], "little")
            assert got < P, "to_raw value %d slot %d: words not below p" % (i, s)
            assert got == val(v[s]) * inv8 % P, "to_raw value %d slot %d: wrong integer" % (i, s)


# ------------------------------------------------------------------------------------------------------------------------------------
# host build of the GENERIC tower on the same raw limbs (tests/host/pairing_host_check.cpp)
_HOST = []


def host_lib():
    if not _HOST:
        import ctypes
        import subprocess

        here = os.path.join(fv.ROOT, "tests", "host")
        so = os.path.join(here, "libpairing_stage_host.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(here, "pairing_host_check.cpp")])
        L = ctypes.CDLL(so)
        L.hp_line_op.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
        L.hp_accumulate_raw.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint, ctypes.c_char_p]
        L.hp_fp12_mul_raw.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]
        _HOST.append(L)
    return _HOST[0]


_HOST_LINE = {}


def host_line_results(name):
    """unpack()ed results of Tower<PF2>::line_dbl / line_add on the vectors of the field op `name` (no sink on the host: the `inf` flag is ignored)"""
    if name not in _HOST_LINE:
        import ctypes

        vecs = fv.vectors(name)
        add = name == "line_add"
        out = ctypes.create_string_buffer(64 * 12 * len(vecs))
        host_lib().hp_line_op(int(add), fv.pack(vecs, 12 if add else 8), len(vecs), out)
        _HOST_LINE[name] = fv.unpack(out.raw, 12)
    return _HOST_LINE[name]


def host_accumulate(m, n):
    import ctypes

    out = ctypes.create_string_buffer(64 * FP12_SLOTS * ((n + m - 1) // m))
    host_lib().hp_accumulate_raw(acc_case(m, n)[1], n, m, out)
    return out.raw


def host_prod(n):
    import ctypes

    vals, res = prod_case(n), b""
    for g in range(n // 2):
        out = ctypes.create_string_buffer(64 * FP12_SLOTS)
        host_lib().hp_fp12_mul_raw(pack_fp12([vals[2 * g]]), pack_fp12([vals[2 * g + 1]]), out)
        res += out.raw
    return res


def timed(fn, *a):
    t = time.time()
    r = fn(*a)
    return r, time.time() - t


# ------------------------------------------------------------------------------------------------------------------------------------
# pairs on the curves but outside the subgroups: the call does not check membership (the reference's Validate::No semantics)
def unchecked_pairs(o):
    """[(name, P, Q, trivial)]: affine points of E(Fp) and E'(Fp2).  Every Q has large order, so no step of the Miller loop meets
    T = +-Q.  trivial: P = (0, +-2) has xP = 0, every line is yP + c w^3, an element of the subfield Fp2[w^3] = Fp4, which the final
    exponentiation sends to one — the pairing value IS one there, whatever the lines were.
    E(Fp) has no point with a coordinate p - 1 (x = p - 1: x^3 + 4 = 3 is not a square; y = p - 1: -3 is not a cube); E'(Fp2) has
    one with x = (p - 1, 0)."""
    from tests import cofactor_util as cu

    P = o.P
    q_sub = o.scalar_mul(o.F2, o.G2_GEN, 0x1234567)
    p_sub = o.scalar_mul(o.F1, o.G1_GEN, 0x7654321)
    off1, off2 = cu.off_subgroup_points(o, "g1", 2), cu.off_subgroup_points(o, "g2", 2)
    xq = (P - 1, 0)
    yq = o.fp2_sqrt(o.F2.add(o.F2.mul(o.F2.mul(xq, xq), xq), o.F2.b))
    assert pow(3, (P - 1) // 2, P) != 1 and pow(P - 3, (P - 1) // 3, P) != 1 and yq is not None
    return [("P=(0,2)", (0, 2), q_sub, True), ("P=(0,p-2)", (0, P - 2), q_sub, True), ("P off the subgroup", off1[0], q_sub, False),
            ("Q off the subgroup", p_sub, off2[0], False), ("both off", off1[1], off2[1], False), ("xQ=(p-1,0)", off1[0], (xq, yq), False),
            ("xQ=(p-1,0), P in G1", p_sub, (xq, yq), False)]
