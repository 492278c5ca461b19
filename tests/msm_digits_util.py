"""Shared by tests/test_msm_digits_cpu.py (CPU) and tests/test_gpu_msm_edges.py (GPU): the signed-digit recoding of the MSM (load_scalar,
for_each_digit_static and for_each_digit, csrc/kernels_common.cuh) restated with Python integers, and the special scalars derived from it.

The kernels cut the canonical integer s < r into c-bit windows, low window first.  A raw digit (window bits + incoming carry) above 2^(c-1)
becomes raw - 2^c and carries one into the next window; the digit d != 0 of window j puts the point into bucket |d| - 1 of that window with
the sign of d.  With the sign fold (validated resident bases only) s > (r - 1) / 2 is replaced by r - s and every sign is inverted; the
value recoded is then below 2^254 and the plan drops the carry-only top window of c = 15 and c = 17 (num_windows, csrc/common.hpp).

What a point-level comparison can and cannot see: a tie recoded as -2^(c-1) with a carry is the same integer (-2^(c-1) + 2^c) and the same
bucket, so the kernels' choice at the tie is a convention this model records, not one a result pins; a wrong result needs a lost carry
(out of the top window, or across a window-group boundary), a wrong sign, or the bucket of magnitude 0."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from batch_mul_util import scalar_bytes  # noqa: E402,F401  (re-exported: the GPU test packs its vectors with it)

C_ALL = tuple(range(7, 23))   # what mi_msm_set_window_bits accepts besides 0

# events of one recoding (recode returns the set that occurred)
TIE = "tie"                        # raw digit == 2^(c-1): stays positive, the LAST bucket of the window
FIRST_NEG = "first_negative"       # raw digit == 2^(c-1) + 1: the first negative one, magnitude 2^(c-1) - 1
ZERO_CARRY = "zero_with_carry"     # raw digit == 2^c (all ones plus the carry): magnitude 0, nothing emitted, the carry goes on
TOP_NONZERO = "top_nonzero"        # the last window of the plan holds a non-zero digit
TOP_CARRY_ONLY = "top_carry_only"  # the last window sees no bit of the value, only the carry of the window below
FLIPPED = "flipped"                # the fold replaced s by r - s


def windows(c, fold):
    return (255 + c - 1) // c + (1 if 255 % c == 0 and not fold else 0)


def recode(v, c, fold, r):
    """(digits, events) of the raw 256-bit value v: digits d_j in [-2^(c-1) + 1, 2^(c-1)], j < windows(c, fold), whose weighted sum is
    v mod r as an integer (without a flip) or v mod r - r (with one).  Asserts that no carry leaves the last window."""
    assert 0 <= v < (1 << 256)
    s = v % r
    events = set()
    flip = fold and s > (r - 1) // 2
    t = r - s if flip else s
    if flip:
        events.add(FLIPPED)
    W, half, full, carry, d = windows(c, fold), 1 << (c - 1), 1 << c, 0, []
    for j in range(W):
        bits = (t >> (c * j)) & (full - 1)
        raw = bits + carry
        if j == W - 1 and (t >> (c * j)) == 0 and carry:
            events.add(TOP_CARRY_ONLY)
        if raw == half:
            events.add(TIE)
        if raw == half + 1:
            events.add(FIRST_NEG)
        if raw == full:
            events.add(ZERO_CARRY)
        neg = raw > half
        carry = 1 if neg else 0
        u = raw - full if neg else raw                       # the digit of t
        assert -half + 1 <= u <= half
        d.append(-u if flip else u)
    assert carry == 0, (hex(v), c, fold)
    assert (t >> (c * W)) == 0, (hex(v), c, fold)            # no bit of the value lies beyond the plan's windows
    if d[-1] != 0:
        events.add(TOP_NONZERO)
    total = sum(x << (c * j) for j, x in enumerate(d))
    assert total == (s - r if flip else s) and total % r == v % r
    return d, events


def _pattern(c, first, rest, limit):
    """digit `first` in window 0 and `rest` in every further window that lies wholly below bit `limit`"""
    out, j = first, 1
    while c * (j + 1) <= limit:
        out |= rest << (c * j)
        j += 1
    return out


def special_scalars(c, r):
    """Raw 256-bit values (the library reduces them modulo r): group-order edges, the fold threshold, every window's digit-sign boundary and
    carry, and whole vectors of tie / first-negative / all-ones digits — once over all 256 bits (reduced by the library, so only the low
    windows keep the pattern) and once below bit 253, where neither the reduction nor the fold touches them."""
    half, full, top = 1 << (c - 1), 1 << c, 1 << 256
    out = [0, 1, 2, r - 2, r - 1, r, r + 1, 2 * r, 2 * r + 1, (r - 1) // 2 - 1, (r - 1) // 2, (r + 1) // 2, (r + 1) // 2 + 1,
           (1 << 255) - 1, top - 1]
    for j in range(windows(c, False) + 1):
        for v in ((1 << (c * j)), (1 << (c * j)) - 1, (1 << (c * j)) >> 1, ((1 << (c * j)) >> 1) + 1):
            if 0 <= v < top:
                out.append(v)
    nw = windows(c, False)
    out.append(sum(half << (c * j) for j in range(nw)) % top)              # every raw digit at the tie (unreduced: the library subtracts r)
    out.append(sum((half + 1) << (c * j) for j in range(nw)) % top)        # every raw digit the first negative one
    out.append(sum((full - 1) << (c * j) for j in range(nw)) % top % r)    # every raw digit all ones, reduced
    out.append(_pattern(c, half, half, 253))                               # all ties, as they stand
    out.append(_pattern(c, half + 1, half + 1, 253))                       # all first-negative: every window carries into the next
    out.append(_pattern(c, half + 1, full - 1, 253))                       # one carry that runs through every window as magnitude 0
    out.append(_pattern(c, half, full - 1, 253))                           # a tie below the same run: no carry starts
    out.append(_pattern(c, half + 1, half - 1, 253))                       # every carry turns the digit above into a tie
    out += [r - x for x in out[-5:]]                                       # the same magnitudes reached through the fold
    return out
