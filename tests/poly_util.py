"""Python big-int reference of opening a polynomial over the BLS12-381 scalar field at a point (mi_fr_poly_open): the value p(z) and the quotient
(p(X) - p(z)) / (X - z) by the serial recurrence S_n = 0, S_i = p_i + z S_(i+1), q_i = S_(i+1), p(z) = S_0 — ark_poly's DensePolynomial::evaluate
and its division by a linear factor.  Shared by test_fr_poly_cpu.py and test_gpu_fr_poly.py; packing comes from ntt_util.  The recurrence pins
itself against the definition and the division identity when the module is imported."""
import builtins
import os
import random
import struct
import subprocess

import ntt_util as nu
from ntt_util import R, expected_bytes, host_exe, pack, pack_raw, raw_of_value, unpack_raw, value_of_raw  # noqa: F401

MAX_N = 1 << 26


def suffix(p, z):
    """[S_0, ..., S_n]: S_i = sum_(j >= i) p_j z^(j - i)"""
    s = [0] * (len(p) + 1)
    for i in range(len(p) - 1, -1, -1):
        s[i] = (p[i] + z * s[i + 1]) % R
    return s


def open(p, z):
    """-> (the quotient with its trailing zero: len(p) elements, p(z))"""
    s = suffix(p, z)
    return s[1:], s[0]


def evaluate(p, z):
    return suffix(p, z)[0]


def sparse_rows(entries, n: int, z: int, rows):
    """Closed form for a polynomial that is zero except entries = {index: coefficient}: the requested elements of the quotient vector
    (row i = S_(i+1) = sum_(j > i) v_j z^(j - i - 1), row n - 1 = 0), each a sum of len(entries) powers (pow), for sizes no loop reaches."""
    assert all(0 <= j < n for j in entries)
    return [sum(v * pow(z, j - i - 1, R) for j, v in entries.items() if j > i) % R for i in rows]


def sparse_value(entries, z: int) -> int:
    return sum(v * pow(z, j, R) for j, v in entries.items()) % R


def levels(n: int, tile_bits: int) -> int:
    """levels of the carry hierarchy: 1 while a polynomial fits one tile, one more for every further division by the tile"""
    lv, m = 1, n
    while m > 1 << tile_bits:
        m = -(-m >> tile_bits)
        lv += 1
    return lv


def run_ref(exe: str, tmpdir: str, data: bytes, n: int, batch: int, points: bytes, fmt: int, threads: int = 1, evaluate_only: bool = False):
    """tests/host/fr_poly_ref.cpp on packed polynomials -> (packed quotients or b"", packed values, seconds of the work alone)"""
    fin, fout = os.path.join(tmpdir, "poly_ref_in.bin"), os.path.join(tmpdir, "poly_ref_out.bin")
    with builtins.open(fin, "wb") as f:   # `open` is the opening of a polynomial here
        f.write(struct.pack("<6I", n, batch, len(points) // 32, fmt, threads, int(evaluate_only)))
        f.write(points)
        f.write(data)
    subprocess.check_call([exe, fin, fout])
    with builtins.open(fout, "rb") as f:
        raw = f.read()
    os.remove(fin)
    os.remove(fout)
    q = 0 if evaluate_only else 32 * n * batch
    assert len(raw) == q + 32 * batch + 8
    return raw[:q], raw[q:q + 32 * batch], struct.unpack("<d", raw[-8:])[0]


def _selfcheck():
    rnd = random.Random(2)
    for n in (0, 1, 2, 3, 7, 33):
        p = [rnd.randrange(R) for _ in range(n)]
        for z in (0, 1, R - 1, rnd.randrange(R)):
            q, v = open(p, z)
            assert v == sum(c * pow(z, j, R) for j, c in enumerate(p)) % R and len(q) == n and (n == 0 or q[-1] == 0)
            x = rnd.randrange(R)   # p(x) - p(z) == q(x) (x - z)
            assert (evaluate(p, x) - v) % R == evaluate(q, x) * (x - z) % R
            ent = {j: p[j] for j in range(0, n, 3)}
            sp = [ent.get(j, 0) for j in range(n)]
            assert sparse_rows(ent, n, z, range(n)) == open(sp, z)[0] and sparse_value(ent, z) == evaluate(sp, z)
    assert [levels(n, 2) for n in (0, 1, 4, 5, 16, 17, 64, 65)] == [1, 1, 1, 2, 2, 3, 3, 4]


_selfcheck()
