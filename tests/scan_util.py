"""Python big-int reference of the batched inversion and the running products / sums over the BLS12-381 scalar field (mi_fr_batch_inverse,
mi_fr_scan): Montgomery's trick with zeros skipped (ark_ff::batch_inversion, batch_inversion_and_mul), the scans as the plain serial loop, the
level count of the tile plan, and closed forms for a vector that is constant except for a few entries.  Shared by test_fr_scan_cpu.py and
test_gpu_fr_scan.py; packing comes from ntt_util.  Everything pins itself against pow(x, -1, R) and the definitions when the module is imported."""
import os
import random
import struct
import subprocess

import ntt_util as nu
from ntt_util import R, expected_bytes, host_exe, pack, pack_raw, raw_of_value, unpack_raw, value_of_raw  # noqa: F401

MAX_N = 1 << 26
MUL, ADD, SUB = 0, 1, 2
MINV = pow(nu.MONT, -1, R)


def values_of_raw(words, fmt: int):
    """value_of_raw for a whole vector (the inverse of 2^256 taken once)"""
    return [w % R * MINV % R for w in words] if fmt else [w % R for w in words]


def batch_inverse(a, num=None):
    """-> ([num[i] / a[i], or 0 where a[i] == 0], the number of zeros): Montgomery's trick, one inversion, zeros skipped"""
    pre, acc = [], 1
    for x in a:
        pre.append(acc)
        if x:
            acc = acc * x % R
    inv = pow(acc, -1, R)
    out = [0] * len(a)
    for i in range(len(a) - 1, -1, -1):
        if a[i]:
            out[i] = inv * pre[i] % R
            inv = inv * a[i] % R
            if num is not None:
                out[i] = out[i] * num[i] % R
    return out, sum(1 for x in a if not x)


def identity(op: int) -> int:
    return 1 if op == MUL else 0


def scan(a, op: int, exclusive: bool):
    """-> (the prefixes, the total)"""
    out, acc = [], identity(op)
    for x in a:
        nxt = acc * x % R if op == MUL else (acc + x) % R
        out.append(acc if exclusive else nxt)
        acc = nxt
    return out, acc


def levels(n: int, tile_bits: int) -> int:
    """levels of the plan: 1 while a vector fits one tile, one more for every further division by the tile"""
    lv, m = 1, n
    while m > 1 << tile_bits:
        m = -(-m >> tile_bits)
        lv += 1
    return lv


# ---- closed forms: a vector of n elements, every one the constant c except specials = {index: value}
def sparse_inverse_rows(c: int, specials, rows, num_c=None, num_specials=None):
    """rows of batch_inverse (with numerators: the constant num_c except num_specials)"""
    cinv = pow(c, -1, R) if c else 0
    out = []
    for i in rows:
        v = specials.get(i, c)
        x = (pow(v, -1, R) if v else 0) if i in specials else cinv
        if num_c is not None:
            x = x * (num_specials or {}).get(i, num_c) % R
        out.append(x)
    return out


def sparse_count(c: int, specials, lo: int, hi: int):
    """(how many of [lo, hi) are the constant, the product and the sum of the specials in it)"""
    inside = [v for j, v in specials.items() if lo <= j < hi]
    prod = 1
    for v in inside:
        prod = prod * v % R
    return hi - lo - len(inside), prod, sum(inside) % R


def sparse_scan_rows(c: int, specials, op: int, exclusive: bool, rows):
    out = []
    for i in rows:
        k, prod, s = sparse_count(c, specials, 0, i if exclusive else i + 1)
        out.append(pow(c, k, R) * prod % R if op == MUL else (c * k + s) % R)
    return out


def sparse_scan_total(c: int, specials, op: int, n: int) -> int:
    return sparse_scan_rows(c, specials, op, True, [n])[0]


# ---- inputs that reach what can go wrong
VARIANTS = ("random", "zeros", "zero_tile", "all_zero", "single_zero", "ones", "minus_one")
ZERO_WORDS = (0, R, 2 * R)   # stored words that reduce to zero, in either format
UNREDUCED = (R + 1, 2 * R + 1, (1 << 256) - 1, 1 << 255)


def make_vector(variant: str, total: int, tile_bits: int, fmt: int, rnd):
    """`total` stored 256-bit words.  random: more than half not below r (every element goes through the load, which reduces).  zeros: a zero as
    first and as last element of a lane, of a wave's span and of a tile, and of the vector, among random words, 1, r - 1 and the unreduced words
    r + 1, 2r + 1, 2^256 - 1, 2^255 (r itself is one of the zeros).  zero_tile: the second tile (the first, if there is only one) all zeros.
    all_zero: nothing else.  single_zero: the word r in the middle.  ones: 1 and r - 1 in turn.  minus_one: r - 1 everywhere."""
    T = 1 << tile_bits
    K = 4 if tile_bits > 8 else 1
    words = unpack_raw(rnd.randbytes(32 * total))
    if variant == "zeros":
        for k, w in enumerate((raw_of_value(1, fmt), raw_of_value(R - 1, fmt)) + UNREDUCED):
            for at in (1 + k, T + 1 + k):
                if at < total:
                    words[at] = w
        for k, at in enumerate((0, K, 2 * K - 1, 64 * K, 128 * K - 1, T - 1, T, 2 * T - 1, total - 1)):
            if 0 <= at < total:
                words[at] = ZERO_WORDS[k % 3]
    elif variant == "zero_tile":
        lo = T if total > T else 0
        for at in range(lo, min(lo + T, total)):
            words[at] = ZERO_WORDS[at % 3]
    elif variant == "all_zero":
        words = [ZERO_WORDS[at % 3] for at in range(total)]
    elif variant == "single_zero":
        if total:
            words[total // 2] = R
    elif variant == "ones":
        words = [raw_of_value(1 if at % 3 else R - 1, fmt) for at in range(total)]
    elif variant == "minus_one":
        words = [raw_of_value(R - 1, fmt)] * total
    else:
        assert variant == "random", variant
    return words



def run_ref(exe: str, tmpdir: str, kind: str, data: bytes, n: int, batch: int = 1, fmt: int = 1, threads: int = 1, op: int = MUL, exclusive: bool = False,
            num: bytes = None, no_out: bool = False):
    """tests/host/fr_scan_ref.cpp on packed vectors -> (packed output or b"", packed totals (scan) or the zero count (inverse), seconds of the
    work alone)"""
    invert = kind == "inverse"
    fin, fout = os.path.join(tmpdir, "scan_ref_in.bin"), os.path.join(tmpdir, "scan_ref_out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<8I", int(invert), n, batch, fmt, threads, op, int(exclusive), (1 if num is not None else 0) | (2 if no_out else 0)))
        f.write(data)
        if num is not None:
            f.write(num)
    subprocess.check_call([exe, fin, fout])
    with open(fout, "rb") as f:
        raw = f.read()
    os.remove(fin)
    os.remove(fout)
    q = 0 if (no_out and not invert) else 32 * n * batch
    secs = struct.unpack("<d", raw[-8:])[0]
    if invert:
        assert len(raw) == q + 16
        return raw[:q], struct.unpack("<Q", raw[q:q + 8])[0], secs
    assert len(raw) == q + 32 * batch + 8
    return raw[:q], raw[q:q + 32 * batch], secs


def _selfcheck():
    rnd = random.Random(3)
    for n in (0, 1, 2, 3, 7, 33):
        a = [rnd.randrange(R) for _ in range(n)]
        for j in range(0, n, 5):
            a[j] = 0
        num = [rnd.randrange(R) for _ in range(n)]
        inv, nz = batch_inverse(a)
        assert nz == len(range(0, n, 5)) and inv == [pow(x, -1, R) if x else 0 for x in a]
        assert batch_inverse(a, num)[0] == [y * pow(x, -1, R) % R if x else 0 for x, y in zip(a, num)]
        for op in (MUL, ADD):
            inc, tot = scan(a, op, False)
            exc, tot2 = scan(a, op, True)
            assert tot == tot2 and exc == [identity(op)] + inc[:-1] if n else (inc, exc, tot) == ([], [], identity(op))
            for i in range(n):
                want = 1 if op == MUL else 0
                for x in a[:i + 1]:
                    want = want * x % R if op == MUL else (want + x) % R
                assert inc[i] == want
        c = rnd.randrange(1, R)
        sp = {j: a[j] for j in range(0, n, 3)}
        v = [sp.get(j, c) for j in range(n)]
        assert sparse_inverse_rows(c, sp, range(n)) == batch_inverse(v)[0]
        assert sparse_inverse_rows(c, sp, range(n), 5, {0: 7}) == batch_inverse(v, [7 if j == 0 else 5 for j in range(n)])[0]
        for op in (MUL, ADD):
            for ex in (False, True):
                assert sparse_scan_rows(c, sp, op, ex, range(n)) == scan(v, op, ex)[0]
            assert sparse_scan_total(c, sp, op, n) == scan(v, op, False)[1]
    assert [levels(n, 2) for n in (0, 1, 4, 5, 16, 17, 64, 65)] == [1, 1, 1, 2, 2, 3, 3, 4]


_selfcheck()
