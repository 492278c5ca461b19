"""Host-side mirror of the reference's operator surface for the MSM path.

Reference (Rust, /root/reference):  impl VariableBaseMSM for G1Projective { fn msm(bases: &[G1Affine],
scalars: &[Scalar]) -> Result<Self, usize> }  (src/g1.rs:602-632; G2: src/g2.rs:582-612), with
`ScalarMul::MulBase = G1Affine` (src/g1.rs:593-600).  Same names and argument meaning here; the Result<_, usize>
error convention is kept: arkworks' generic entry returns Err(min(len)) on a length mismatch and the
reference's GPU impl returns Err(0) for any device failure (src/g1.rs:628-630) — mirrored by MsmErr.
"""
from __future__ import annotations

from .binding import Context, FR_MUL, MsmError, SCALAR_CANONICAL, SCALAR_MONTGOMERY

_default_ctx = None


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context()
        # the trait call carries no handle: keep the device form of the last two base vectors (mi_msm_set_base_cache, include/arkblst_amd.h:
        # keyed by a fingerprint of every byte of the vector, so msm() stays a function of its arguments); ARKBLST_AMD_BASE_CACHE=0 in the
        # environment switches it off
        _default_ctx.set_base_cache(2)
    return _default_ctx


class MsmErr(Exception):
    """Err(usize) of the reference's Result: .value = min(len) on length mismatch, 0 on a GPU failure."""

    def __init__(self, value: int, detail: str = ""):
        self.value = value
        super().__init__(f"Err({value}) {detail}")


class _Projective:
    GROUP = ""
    AFFINE_BYTES = 0

    @classmethod
    def msm(cls, bases: bytes, scalars: bytes, *, scalar_fmt: int = SCALAR_MONTGOMERY, ctx: Context | None = None) -> bytes:
        """bases: packed blst affine points; scalars: packed 32-byte `Scalar`s (Montgomery blst_fr, the in-memory
        form of the reference's `Scalar`, by default).  Returns the projective result (blst_p1 / blst_p2 bytes)."""
        nb, ns = len(bases) // cls.AFFINE_BYTES, len(scalars) // 32
        if nb != ns:
            raise MsmErr(min(nb, ns), "bases and scalars differ in length")
        try:
            return (ctx or default_context()).msm(cls.GROUP, bases, scalars, nb, scalar_fmt)
        except MsmError as e:
            raise MsmErr(0, str(e)) from e

    @classmethod
    def msm_bigint(cls, bases: bytes, bigints: bytes, *, ctx: Context | None = None) -> bytes:
        """arkworks' msm_bigint: scalars already canonical BigInteger256 (what src/g1.rs:624-627 builds)."""
        return cls.msm(bases, bigints, scalar_fmt=SCALAR_CANONICAL, ctx=ctx)

    @classmethod
    def batch_mul(cls, base: bytes, scalars: bytes, *, scalar_fmt: int = SCALAR_MONTGOMERY, ctx: Context | None = None) -> bytes:
        """ark_ec's ScalarMul::batch_mul / FixedBase::msm + normalize_batch, which the reference leaves to the arkworks defaults on the CPU
        (`impl ScalarMul`, src/g1.rs:593-600, src/g2.rs:573-580): base = one packed affine point, scalars = packed 32-byte `Scalar`s.
        Returns the packed affine points scalars[i] * base."""
        if len(base) != cls.AFFINE_BYTES or len(scalars) % 32:
            raise MsmErr(0, "base must be one affine point and scalars a whole number of 32-byte values")
        try:
            return (ctx or default_context()).batch_mul(cls.GROUP, base, scalars, scalar_fmt)
        except MsmError as e:
            raise MsmErr(0, str(e)) from e


class G1Projective(_Projective):
    GROUP = "g1"
    AFFINE_BYTES = 96


class G2Projective(_Projective):
    GROUP = "g2"
    AFFINE_BYTES = 192


class Radix2EvaluationDomain:
    """ark_poly::Radix2EvaluationDomain<Scalar> over the GPU transform (mi_fr_ntt).  The reference makes `Scalar` an FftField
    (src/scalar.rs:465-470) and leaves fft / ifft / coset_fft / coset_ifft to ark-poly's generic code on the CPU; that code has no trait
    method to override, so a prover calls this mirror instead.  Vectors are packed 32-byte `Scalar`s, Montgomery blst_fr by default."""

    MAX_LOG_SIZE = 26
    GENERATOR = 7   # FftField::GENERATOR: arkworks' default coset offset

    def __init__(self, log_size: int, ctx: Context | None = None):
        self.log_size_of_group = log_size
        self.size = 1 << log_size
        self._ctx = ctx

    @classmethod
    def new(cls, num_coeffs: int, ctx: Context | None = None):
        """The smallest power-of-two domain that holds num_coeffs coefficients, or None when that is more than 2^26 elements."""
        log_size = max(num_coeffs - 1, 0).bit_length()
        return cls(log_size, ctx) if log_size <= cls.MAX_LOG_SIZE else None

    @staticmethod
    def _scalar(value: int, scalar_fmt: int) -> bytes:
        r = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
        return ((value << 256) % r if scalar_fmt == SCALAR_MONTGOMERY else value % r).to_bytes(32, "little")

    def _run(self, data: bytes, inverse: bool, offset, scalar_fmt: int) -> bytes:
        if len(data) % 32 or len(data) > 32 * self.size:
            raise MsmErr(0, "the input must be whole 32-byte scalars and no longer than the domain")
        data = bytes(data) + bytes(32 * self.size - len(data))   # arkworks resizes a shorter input with zeros
        if isinstance(offset, int):
            offset = self._scalar(offset, scalar_fmt)
        try:
            return (self._ctx or default_context()).fr_ntt(data, self.log_size_of_group, 1, inverse, offset, scalar_fmt)
        except MsmError as e:
            raise MsmErr(0, str(e)) from e

    def fft(self, coeffs: bytes, *, scalar_fmt: int = SCALAR_MONTGOMERY) -> bytes:
        return self._run(coeffs, False, None, scalar_fmt)

    def ifft(self, evals: bytes, *, scalar_fmt: int = SCALAR_MONTGOMERY) -> bytes:
        return self._run(evals, True, None, scalar_fmt)

    def coset_fft(self, coeffs: bytes, offset=GENERATOR, *, scalar_fmt: int = SCALAR_MONTGOMERY) -> bytes:
        """offset: an integer, or 32 bytes in scalar_fmt"""
        return self._run(coeffs, False, offset, scalar_fmt)

    def coset_ifft(self, evals: bytes, offset=GENERATOR, *, scalar_fmt: int = SCALAR_MONTGOMERY) -> bytes:
        return self._run(evals, True, offset, scalar_fmt)


class DensePolynomial:
    """ark_poly::univariate::DensePolynomial<Scalar> where a KZG / Marlin / PLONK prover opens a commitment: `evaluate`, the division by
    (X - z) that ark-poly-commit's KZG10::compute_witness_polynomial runs on one CPU thread, and the opening itself on device-resident
    coefficients (mi_fr_poly_open).  coeffs: packed 32-byte `Scalar`s in ascending order, Montgomery blst_fr by default; a point is an
    integer or 32 bytes in scalar_fmt."""

    MAX_COEFFS = 1 << 26

    def __init__(self, coeffs: bytes, *, scalar_fmt: int = SCALAR_MONTGOMERY, ctx: Context | None = None):
        if len(coeffs) % 32 or len(coeffs) > 32 * self.MAX_COEFFS:
            raise MsmErr(0, "the coefficients must be whole 32-byte scalars, at most 2^26 of them")
        self.coeffs = bytes(coeffs)
        self.scalar_fmt = scalar_fmt
        self._ctx = ctx

    def __len__(self) -> int:
        return len(self.coeffs) // 32

    @staticmethod
    def _point(point, scalar_fmt: int) -> bytes:
        if isinstance(point, int):
            return Radix2EvaluationDomain._scalar(point, scalar_fmt)
        if len(point) != 32:
            raise MsmErr(0, "a point is one 32-byte scalar")
        return bytes(point)

    def _open(self, point, quotients: bool):
        z = self._point(point, self.scalar_fmt)
        if not self.coeffs:   # the zero polynomial
            return b"", bytes(32)
        try:
            return (self._ctx or default_context()).fr_poly_open(self.coeffs, len(self), 1, z, self.scalar_fmt, quotients=quotients)
        except MsmError as e:
            raise MsmErr(0, str(e)) from e

    def evaluate(self, point) -> bytes:
        """fn evaluate(&self, point: &F) -> F, as 32 bytes in scalar_fmt"""
        return self._open(point, False)[1]

    def divide_by_linear(self, point):
        """-> (quotient, value): (p(X) - p(z)) / (X - z), one coefficient shorter than p, and p(z)"""
        q, v = self._open(point, True)
        return DensePolynomial(q[:-32], scalar_fmt=self.scalar_fmt, ctx=self._ctx), v

    @staticmethod
    def kzg10_open(ctx: Context, d_coeffs_ptr: int, n: int, point, *, scalar_fmt: int = SCALAR_MONTGOMERY, d_quotient_ptr: int | None = None):
        """KZG10::open on n coefficients in DEVICE memory over the n resident G1 bases of ctx (the SRS): divides by (X - point) on the device and
        runs msm_device on the quotient as it is (its last element is zero).  Returns (proof = the Jacobian point [q(tau)]G, value = p(point)).
        d_quotient_ptr: n x 32 bytes of device memory for the quotient; None divides IN PLACE, the coefficients are replaced by the quotient."""
        if n < 1 or n > DensePolynomial.MAX_COEFFS:
            raise MsmErr(0, "n must be between 1 and 2^26")
        z = DensePolynomial._point(point, scalar_fmt)
        d_q = d_coeffs_ptr if d_quotient_ptr is None else d_quotient_ptr
        try:
            value = ctx.fr_poly_open_device(d_coeffs_ptr, n, 1, z, scalar_fmt, d_q)
            return ctx.msm_device("g1", d_q, n, scalar_fmt), value
        except MsmError as e:
            raise MsmErr(0, str(e)) from e


MAX_BATCH_INVERSION = 1 << 26   # elements of one library call; longer vectors go through in pieces (the operation is element-wise)


def _inversion(v: bytes, num, scalar_fmt: int, ctx: Context | None):
    if len(v) % 32 or (num is not None and len(num) != len(v)):
        raise MsmErr(0, "the vectors must be whole 32-byte scalars of the same length")
    out, zeros, step = [], 0, 32 * MAX_BATCH_INVERSION
    try:
        for lo in range(0, len(v), step):
            o, z = (ctx or default_context()).fr_batch_inverse(v[lo:lo + step], None if num is None else num[lo:lo + step], scalar_fmt)
            out.append(o)
            zeros += z
    except MsmError as e:
        raise MsmErr(0, str(e)) from e
    return b"".join(out), zeros


def batch_inversion(v: bytes, *, scalar_fmt: int = SCALAR_MONTGOMERY, ctx: Context | None = None) -> bytes:
    """ark_ff::batch_inversion(&mut v): every non-zero element of v (packed 32-byte `Scalar`s) replaced by its inverse, zeros left as they are
    (mi_fr_batch_inverse).  Returns the new vector."""
    return _inversion(v, None, scalar_fmt, ctx)[0]


def batch_inversion_and_mul(v: bytes, coeffs: bytes, *, scalar_fmt: int = SCALAR_MONTGOMERY, ctx: Context | None = None) -> bytes:
    """ark_ff::batch_inversion_and_mul with a multiplier per element — coeffs[i] / v[i], zero where v[i] is zero: the element-wise quotient of two
    evaluation vectors (ark-poly's Evaluations / Evaluations).  coeffs of 32 bytes is arkworks' one coefficient for every element."""
    if len(coeffs) == 32 and len(v) != 32:
        coeffs = bytes(coeffs) * (len(v) // 32)
    return _inversion(v, coeffs, scalar_fmt, ctx)[0]


def grand_product(ctx: Context, d_num_ptr: int, d_den_ptr: int, n: int, d_out_ptr: int, *, scalar_fmt: int = SCALAR_MONTGOMERY):
    """The running product of a permutation argument on vectors in DEVICE memory: z[0] = 1, z[i+1] = z[i] num[i] / den[i], i < n, written to the n
    elements at d_out_ptr (which may be d_num_ptr or d_den_ptr) — mi_fr_batch_inverse_device with the numerators, then the exclusive product
    scan in place.  Returns (total, n_zero): the product of all n quotients (32 bytes in scalar_fmt; one for a permutation argument that holds)
    and the number of zero denominators (their quotients count as zero)."""
    if n < 1 or n > MAX_BATCH_INVERSION:
        raise MsmErr(0, "n must be between 1 and 2^26")
    try:
        zeros = ctx.fr_batch_inverse_device(d_den_ptr, d_num_ptr, n, scalar_fmt, d_out_ptr)
        return ctx.fr_scan_device(FR_MUL, d_out_ptr, n, 1, True, scalar_fmt, d_out_ptr), zeros
    except MsmError as e:
        raise MsmErr(0, str(e)) from e
