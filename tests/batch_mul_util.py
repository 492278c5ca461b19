"""Shared by tests/test_batch_mul_cpu.py (CPU) and tests/test_gpu_batch_mul.py (GPU): the signed-digit recoding of the fixed-base
batch multiplication restated with Python integers, and the special scalars derived from it.

Table of window size w: T[j][m - 1] = m 2^(w j) P, j < W = windows(w).  A lane adds the entries of the non-zero digits of s, low
window first.  xyzz_madd only DETECTS an exceptional pair (running sum == +- entry); the lane then finishes on complete additions."""

W_SUPPORTED = tuple(range(8, 17))   # what mi_batch_mul_set_window_bits accepts besides 0 (fixed_base_model.hpp W_MIN .. W_MAX)


def windows(w):
    return (255 + w - 1) // w + (1 if 255 % w == 0 else 0)


def recode(s, w):
    """signed digits d_j in [-2^(w-1) + 1, 2^(w-1)] with sum d_j 2^(w j) == s, for 0 <= s < r"""
    W, half, carry, d = windows(w), 1 << (w - 1), 0, []
    for j in range(W):
        raw = ((s >> (w * j)) & ((1 << w) - 1)) + carry
        neg = raw > half
        carry = 1 if neg else 0
        d.append(raw - (1 << w) if neg else raw)
    assert carry == 0 and sum(x << (w * j) for j, x in enumerate(d)) == s
    return d


def collision_scalar(w, r):
    """The scalar below r whose walk on a base of prime order r meets an exceptional pair, or None when w has none.

    An exceptional pair needs running sum v P == +- t B P with v = sum of the digits below window j and t B = d_j 2^(w j).  Below the
    top window |v| < 2^(w j) <= |t B| < r / 2, so the two agree modulo r only as integers, which the sizes exclude.  At the top window
    B = 2^(w (W - 1)) and v = t B - r is possible when t B is the multiple of B next to r: r = q B + rho, and
      * t = q, v = -rho needs rho within the low windows' signed range (about B / 2): the scalar is s = v + q B = r - 2 rho, the
        running sum -rho P EQUALS the entry (r - rho) P and the last addition is a doubling;
      * t = q + 1, v = B - rho gives s = r + 2 v >= r, which load_scalar reduces to 2 v first: no collision;
      * running sum == -entry means s == 0 modulo r, which is recoded as zero: cancellation cannot happen on a prime-order base (bases
        of order 3 or 11 reach it at almost every step).
    So exactly the w with rho <= the low range have one scalar: w = 9, 12 and 14 of the supported sizes."""
    W = windows(w)
    B = 1 << (w * (W - 1))
    q, rho = divmod(r, B)
    s = r - 2 * rho
    if s <= 0:
        return None
    d = recode(s, w)
    v = sum(x << (w * j) for j, x in enumerate(d[:-1]))
    if d[-1] * B != r + v:       # the top entry is not congruent to the running sum
        return None
    assert v == -rho and d[-1] == q and (d[-1] * B - v) % r == 0
    return s


def special_scalars(w, r):
    """Raw 256-bit values (reduced modulo r by the library): group-order edges, every window's digit-sign boundary and carry chain, every
    digit at the half value, and the constructed collisions of EVERY supported window size (so one list serves every table geometry)."""
    out = [0, 1, 2, r - 1, r, r + 1, (r - 1) // 2, (r + 1) // 2, (1 << 255) - 1, (1 << 256) - 1]
    for j in range(windows(w)):
        for v in ((1 << (w * j)), (1 << (w * j)) - 1, (1 << (w * j)) >> 1, ((1 << (w * j)) >> 1) + 1):
            if 0 <= v < (1 << 256):
                out.append(v)
    out.append(sum((1 << (w - 1)) << (w * j) for j in range(windows(w))) % (1 << 256))   # every raw digit at the half value
    for ww in W_SUPPORTED:
        s = collision_scalar(ww, r)
        if s is not None:
            B = 1 << (ww * (windows(ww) - 1))
            out += [s, r - s, s + r if s + r < (1 << 256) else s]     # the collision, its negative, and the same scalar unreduced
            out += [(r + 2 * (B - r % B)) % (1 << 256)]                # the t = q + 1 candidate, which reduces to a plain scalar
    return out


def scalar_bytes(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)
