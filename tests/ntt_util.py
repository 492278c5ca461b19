"""Python big-int reference of the radix-2 NTT over the BLS12-381 scalar field, in the convention of ark_poly::Radix2EvaluationDomain<Scalar>
(natural order in and out; GENERATOR = 7, TWO_ADICITY = 32, reference src/scalar.rs:465-470), shared by test_fr_ntt_cpu.py and
test_gpu_fr_ntt.py.  The iterative transform pins itself against the O(n^2) definition for log_n <= 5 when the module is imported."""
import os
import random
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT_DIR = os.path.dirname(HERE)
if ROOT_DIR not in sys.path:
    sys.path.insert(0, ROOT_DIR)
from oracle import bls12_381 as o  # noqa: E402

R = o.R_ORDER
GENERATOR = 7
TWO_ADICITY = 32
ROOT = pow(GENERATOR, (R - 1) >> TWO_ADICITY, R)   # the 2^32-th root of unity
MONT = 1 << 256
MAX_LOG_N = 26


def omega(log_n: int, inverse: bool = False) -> int:
    w = pow(ROOT, 1 << (TWO_ADICITY - log_n), R)
    return pow(w, -1, R) if inverse else w


def ntt(a, w):
    """out[k] = sum_j a[j] w^(jk) for len(a) = 2^L and w of that order: bit reversal, then L in-place decimation-in-time levels"""
    n = len(a)
    L = n.bit_length() - 1
    assert n == 1 << L
    out = [a[int(format(i, f"0{L}b")[::-1], 2)] if L else a[i] for i in range(n)]
    half = 1
    while half < n:
        step = pow(w, n // (2 * half), R)
        tw = [1] * half
        for i in range(1, half):
            tw[i] = tw[i - 1] * step % R
        for start in range(0, n, 2 * half):
            for i in range(half):
                x, y = out[start + i], out[start + i + half] * tw[i] % R
                out[start + i], out[start + i + half] = (x + y) % R, (x - y) % R
        half *= 2
    return out


def dft(a, w):
    """the definition, O(n^2)"""
    n = len(a)
    return [sum(a[j] * pow(w, j * k, R) for j in range(n)) % R for k in range(n)]


def fft(a):
    return ntt(a, omega(len(a).bit_length() - 1))


def ifft(a):
    n = len(a)
    ninv = pow(n, -1, R)
    return [x * ninv % R for x in ntt(a, omega(n.bit_length() - 1, True))]


def _scaled_by_powers(a, g):
    out, p = [], 1
    for x in a:
        out.append(x * p % R)
        p = p * g % R
    return out


def coset_fft(a, g=GENERATOR):
    return fft(_scaled_by_powers(a, g))


def coset_ifft(a, g=GENERATOR):
    return _scaled_by_powers(ifft(a), pow(g, -1, R))


def transform(a, inverse: bool, offset=None):
    """the operation mi_fr_ntt(inverse, coset_offset) computes on one vector of residues"""
    if offset is None:
        return ifft(a) if inverse else fft(a)
    return coset_ifft(a, offset) if inverse else coset_fft(a, offset)


def sparse_rows(entries, log_n: int, rows, inverse: bool, offset=None):
    """Closed form for a vector that is zero except entries = {index: value}: the requested output rows of transform(), each a sum of
    len(entries) powers (pow), for sizes no table reaches."""
    n = 1 << log_n
    w = omega(log_n, inverse)
    ninv = pow(n, -1, R)
    out = []
    for k in rows:
        if inverse:
            v = sum(x * pow(w, j * k, R) for j, x in entries.items()) * ninv
            if offset is not None:
                v *= pow(offset, -k, R)
        else:
            v = sum(x * (pow(offset, j, R) if offset is not None else 1) * pow(w, j * k, R) for j, x in entries.items())
        out.append(v % R)
    return out


# ---- packing: fmt 0 = canonical integers, 1 = Montgomery blst_fr (the in-memory form of the reference's Scalar)
def pack(vals, fmt: int) -> bytes:
    """residues -> packed scalars in fmt"""
    return b"".join((o.fr_to_mont_bytes(v) if fmt else o.fr_to_canon_bytes(v)) for v in vals)


def pack_raw(words) -> bytes:
    """the 256-bit values exactly as given (non-reduced inputs)"""
    return b"".join(int(v).to_bytes(32, "little") for v in words)


def unpack_raw(b: bytes):
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def value_of_raw(word: int, fmt: int) -> int:
    """the residue a stored 256-bit word stands for: reduced modulo r, and taken out of Montgomery form for fmt 1"""
    return (word % R) * pow(MONT, -1, R) % R if fmt else word % R


def raw_of_value(v: int, fmt: int) -> int:
    """the fully reduced word the library stores for the residue v"""
    return v % R * MONT % R if fmt else v % R


def expected_bytes(vals, fmt: int) -> bytes:
    return pack_raw(raw_of_value(v, fmt) for v in vals)


# ---- operands of the element tests (issue: every pair of these, plus 200 random pairs)
def edge_operands():
    """stored 256-bit words (two of them are not below r: every operand goes through the load, which reduces)"""
    ops = [0, 1, 2, R - 1, R - 2, (R - 1) // 2, MONT % R, 1 << 255, ((R >> 224) << 224) | ((1 << 224) - 1)]
    return ops + [1 << (32 * k) for k in range(1, 8)]


def load_only_operands():
    return [R, R + 1, 2 * R, 2 * R + 1, (1 << 256) - 1]


def host_exe(name: str, sanitize: bool = False) -> str:
    """tests/host/<name>.cpp built as a stand-alone program (g++), optionally under AddressSanitizer + UBSan"""
    exe = os.path.join(HERE, "host", name + ("_san" if sanitize else ""))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-pthread", *flags, "-o", exe, os.path.join(HERE, "host", name + ".cpp")])
    return exe


def run_ref(exe: str, tmpdir: str, data: bytes, log_n: int, batch: int, inverse: bool, offset_bytes, fmt: int, threads: int = 1):
    """tests/host/fr_ntt_ref.cpp on packed vectors -> (packed result, seconds of the transforms alone)"""
    import struct

    fin, fout = os.path.join(tmpdir, "ref_in.bin"), os.path.join(tmpdir, "ref_out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<6I", log_n, batch, int(inverse), int(offset_bytes is not None), fmt, threads))
        f.write(offset_bytes if offset_bytes is not None else bytes(32))
        f.write(data)
    subprocess.check_call([exe, fin, fout])
    raw = open(fout, "rb").read()
    os.remove(fin)
    os.remove(fout)
    assert len(raw) == len(data) + 8
    return raw[:-8], struct.unpack("<d", raw[-8:])[0]


def _selfcheck():
    rnd = random.Random(1)
    for L in range(0, 6):
        a = [rnd.randrange(R) for _ in range(1 << L)]
        assert fft(a) == dft(a, omega(L)), L
        ninv = pow(1 << L, -1, R)
        assert ifft(a) == [x * ninv % R for x in dft(a, omega(L, True))], L
        assert ifft(fft(a)) == a and coset_ifft(coset_fft(a, 5), 5) == a
        g = rnd.randrange(1, R)
        assert coset_fft(a, g) == dft([x * pow(g, j, R) % R for j, x in enumerate(a)], omega(L)), L
        ent = {j: a[j] for j in range(0, 1 << L, 3)}
        sp = [ent.get(j, 0) for j in range(1 << L)]
        for inv in (False, True):
            for off in (None, g):
                assert sparse_rows(ent, L, range(1 << L), inv, off) == transform(sp, inv, off), (L, inv)
    assert pow(ROOT, 1 << 32, R) == 1 and pow(ROOT, 1 << 31, R) == R - 1


_selfcheck()
