"""Reference side of the NTT over G1 points (mi_g1_ntt), shared by test_g1_ntt_cpu.py and test_gpu_g1_ntt.py: the definition computed by the C
oracle (one naive MSM per output row), the closed form for a powers-of-tau input, the non-adjacent form of an integer, and the runner of
tests/host/g1_ntt_host.cpp.  Scalars are Python integers modulo r; points are packed affine bytes (96 B, infinity = zeros)."""
import os
import struct
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ntt_util as nu  # noqa: E402

R = nu.R
AFF, JAC = 96, 144
INF = bytes(AFF)
MAX_LOG_N = 24


def naf(t: int):
    """-> (pos, neg): t = sum_i (pos_i - neg_i) 2^i with no two neighbouring digits non-zero (the textbook right-to-left loop)"""
    pos = neg = 0
    i = 0
    while t:
        if t & 1:
            d = 2 - (t & 3)   # 1 or -1, chosen so that the next bit becomes zero
            t -= d
            if d > 0:
                pos |= 1 << i
            else:
                neg |= 1 << i
        t >>= 1
        i += 1
    return pos, neg


def recoding_cases(rnd):
    vals = [0, 1, 2, R - 1, (R - 1) // 2, (R + 1) // 2]
    for log_n in range(1, 7):
        for inverse in (False, True):
            w = nu.omega(log_n, inverse)
            vals += [pow(w, e, R) for e in range(1 << (log_n - 1))]
    return vals + [rnd.randrange(R) for _ in range(256)]


def host_exe(sanitize: bool = False) -> str:
    """tests/host/g1_ntt_host.cpp built as a stand-alone program (g++; ec.cuh and fp28.cuh carry the device compiler's unroll pragmas),
    optionally under AddressSanitizer + UBSan"""
    exe = os.path.join(HERE, "host", "g1_ntt_host" + ("_san" if sanitize else ""))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", *flags, "-o", exe, os.path.join(HERE, "host", "g1_ntt_host.cpp")])
    return exe


def host_recode(exe: str, tmpdir: str, vals):
    fin, fout = os.path.join(tmpdir, "rec_in.bin"), os.path.join(tmpdir, "rec_out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<I", len(vals)))
        for v in vals:
            f.write(int(v).to_bytes(32, "little"))
    subprocess.check_call([exe, "recode", fin, fout])
    raw = open(fout, "rb").read()
    assert len(raw) == 64 * len(vals)
    return [(int.from_bytes(raw[64 * k:64 * k + 32], "little"), int.from_bytes(raw[64 * k + 32:64 * k + 64], "little")) for k in range(len(vals))]


def host_transform(co, exe: str, tmpdir: str, cases):
    """cases: [(log_n, inverse, points)] -> the transforms as packed affine points (the program's Jacobian output through the oracle's to_affine)"""
    fin, fout = os.path.join(tmpdir, "tr_in.bin"), os.path.join(tmpdir, "tr_out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for log_n, inverse, pts in cases:
            assert len(pts) == AFF << log_n
            f.write(struct.pack("<2I", log_n, int(inverse)))
            f.write(pts)
    subprocess.check_call([exe, "transform", fin, fout])
    raw = open(fout, "rb").read()
    outs, pos = [], 0
    for log_n, inverse, pts in cases:
        if log_n == 0:
            outs.append(raw[pos:pos + AFF])
            pos += AFF
            continue
        n = 1 << log_n
        outs.append(b"".join(co.to_affine("g1", raw[pos + JAC * k:pos + JAC * (k + 1)]) for k in range(n)))
        pos += JAC * n
    assert pos == len(raw)
    return outs


def ref_exe() -> str:
    """tests/host/g1_ntt_ref.c: the CPU baseline over the oracle's point arithmetic (gcc)"""
    exe = os.path.join(HERE, "host", "g1_ntt_ref")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-pthread", "-o", exe, os.path.join(HERE, "host", "g1_ntt_ref.c")])
    return exe


def run_ref(exe: str, tmpdir: str, pts: bytes, log_n: int, inverse: bool, threads: int = 1):
    """-> (the transform as packed Jacobian points of the oracle, seconds of the transform alone); log_n >= 1"""
    n = 1 << log_n
    w = nu.omega(log_n, inverse)
    fin, fout = os.path.join(tmpdir, "g1ref_in.bin"), os.path.join(tmpdir, "g1ref_out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<4I", log_n, int(inverse), threads, 0))
        f.write(pack_scalars(powers(w, n // 2) + [pow(n, -1, R)]))
        f.write(pts)
    subprocess.check_call([exe, fin, fout])
    raw = open(fout, "rb").read()
    os.remove(fin)
    os.remove(fout)
    assert len(raw) == JAC * n + 8
    return raw[:-8], struct.unpack("<d", raw[-8:])[0]


def point(pts: bytes, j: int) -> bytes:
    return pts[AFF * j:AFF * (j + 1)]


def combination(co, pts: bytes, scalars) -> bytes:
    """sum_j [scalars[j]] P_j as a packed affine point: one naive MSM of the oracle over the finite points"""
    keep = [j for j in range(len(scalars)) if point(pts, j) != INF and scalars[j] % R]
    if not keep:
        return INF
    bases = b"".join(point(pts, j) for j in keep)
    sc = b"".join((scalars[j] % R).to_bytes(32, "little") for j in keep)
    return co.to_affine("g1", co.msm_naive("g1", bases, sc, len(keep), 0))


def definition(co, pts: bytes, log_n: int, inverse: bool, rows=None) -> bytes:
    """out[k] = sum_j [w^(jk)] P_j, or [1 / n] sum_j [w^(-jk)] P_j: the rows asked for (all of them by default), back to back"""
    n = 1 << log_n
    w = nu.omega(log_n, inverse)
    scale = pow(n, -1, R) if inverse else 1
    out = []
    for k in (range(n) if rows is None else rows):
        wk = pow(w, k, R)
        sc, p = [], scale
        for _ in range(n):
            sc.append(p)
            p = p * wk % R
        out.append(combination(co, pts, sc))
    return b"".join(out)


def batch_inverse(vals):
    """Montgomery's trick: every 1 / v with one modular inversion (no v is zero)"""
    pre, run = [], 1
    for v in vals:
        pre.append(run)
        run = run * v % R
    inv = pow(run, -1, R)
    out = [0] * len(vals)
    for k in range(len(vals) - 1, -1, -1):
        out[k] = inv * pre[k] % R
        inv = inv * vals[k] % R
    return out


def closed_form_scalars(tau: int, log_n: int, inverse: bool):
    """the transform of P_j = [tau^j] G is [c_k] G with
    forward: c_k = (tau^n - 1) / (tau w^k - 1);   inverse: c_k = (tau^n - 1) w^k / (n (tau - w^k)),   w = omega(log_n)"""
    n = 1 << log_n
    w = nu.omega(log_n)
    top = (pow(tau, n, R) - 1) % R
    wk, p = [], 1
    for _ in range(n):
        wk.append(p)
        p = p * w % R
    if inverse:
        den = batch_inverse([n * (tau - x) % R for x in wk])
        return [top * x % R * d % R for x, d in zip(wk, den)]
    den = batch_inverse([(tau * x - 1) % R for x in wk])
    return [top * d % R for d in den]


def powers(tau: int, n: int):
    out, p = [], 1
    for _ in range(n):
        out.append(p)
        p = p * tau % R
    return out


def pack_scalars(vals) -> bytes:
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


def _selfcheck():
    import random

    rnd = random.Random(5)
    for t in (0, 1, 2, 3, 7, R - 1, rnd.randrange(R)):
        p, m = naf(t)
        assert p - m == t and not (p & m) and not ((p | m) & ((p | m) >> 1)) and (p | m) < 1 << 256
    tau = rnd.randrange(2, R)
    for log_n in (1, 3, 6):   # both identities against the scalar transform of the powers of tau
        for inverse in (False, True):
            assert closed_form_scalars(tau, log_n, inverse) == nu.transform(powers(tau, 1 << log_n), inverse), (log_n, inverse)


_selfcheck()
