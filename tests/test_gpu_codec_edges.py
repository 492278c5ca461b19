"""GPU tests of the point codec (csrc/codec_kernels.cuh) on the edge fixtures of tests/golden/msm_vectors.json: G2 points whose curve
right-hand side lies in Fp (the a1 == 0 branch of fp2_sqrt_complex; y real, where fp2_lex_largest falls back to c0, or purely
imaginary), the G1 point (0, 2) of order 3, and batches that mix accepted and rejected encodings at every lane parity.  The single
fixtures themselves run through tests/test_gpu_msm.py::test_g1_deserialize_golden and ::test_g2_deserialize_golden_and_roundtrip."""
import ctypes as C
import json
import os

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GROUPS = ["g1", "g2"]


def _golden():
    with open(os.path.join(HERE, "golden", "msm_vectors.json")) as f:
        return json.load(f)


def _curve(o, group):
    return (o.F1, 96, 48) if group == "g1" else (o.F2, 192, 96)


def _mixed_batch(group):
    """every compressed, validated fixture of the group, repeated to more than 300 entries in rounds of ODD length: each fixture comes
    by at even and at odd positions (the two lanes of a pair of k_validate_g2_coop) with changing neighbours"""
    comp = [c for c in _golden()[f"{group}_encoding"] if c["compressed"] and c["validate"]]
    assert {c["status"] for c in comp} == {0, 1, 3}
    if len(comp) % 2:
        comp = comp + comp[:1]
    out = []
    for rep in range(-(-300 // (len(comp) + 1))):
        k = 2 * rep % len(comp)      # an even rotation in rounds of odd length: the parity of a fixture's position changes every round
        out += comp[k:] + comp[:k] + [comp[(3 * rep) % len(comp)]]
    assert len(out) >= 300
    for c in comp:
        assert {i % 2 for i, x in enumerate(out) if x is c} == {0, 1}, c["name"]
    return out


def test_serializer_on_the_edge_points(ctx, o):
    """compress: the sort flag of a G2 point with y.c1 == 0 comes from y.c0; (0, +-2) on G1"""
    cases = {c["name"]: c for c in _golden()["g2_encoding"]}
    pts = []
    for kind in ("y_real", "y_imaginary"):
        pt = o.affine_from_bytes(o.F2, bytes.fromhex(cases[f"rhs_in_fp_{kind}_compressed_unvalidated"]["affine"]))
        assert pt[1][1 if kind == "y_real" else 0] == 0
        pts += [pt, (pt[0], o.F2.neg(pt[1]))]
    raw = b"".join(o.affine_to_bytes(o.F2, p) for p in pts)
    want = b"".join(o.g2_compress(p) for p in pts)
    assert {want[96 * i] & 0x20 for i in (0, 1)} == {0, 0x20} and {want[96 * i] & 0x20 for i in (2, 3)} == {0, 0x20}
    assert ctx.serialize_batch("g2", raw, True) == want
    assert ctx.serialize_batch("g2", raw, False) == b"".join(o.g2_uncompressed(p) for p in pts)
    dec, st = ctx.deserialize_batch("g2", want, True, False)
    assert st == bytes(4) and dec == raw
    g1 = [(0, 2), (0, o.P - 2)]
    raw1 = b"".join(o.affine_to_bytes(o.F1, p) for p in g1)
    want1 = b"".join(o.g1_compress(p) for p in g1)
    assert want1[0] & 0x20 == 0 and want1[48] & 0x20 == 0x20
    assert ctx.serialize_batch("g1", raw1, True) == want1
    assert ctx.serialize_batch("g1", raw1, False) == b"".join(o.g1_uncompressed(p) for p in g1)
    dec, st = ctx.deserialize_batch("g1", want1, True, False)
    assert st == bytes(2) and dec == raw1


@pytest.mark.parametrize("group", GROUPS)
def test_deserialize_mixed_batch_keeps_per_element_status(ctx, o, group):
    """valid, infinity, malformed and off-subgroup encodings side by side over several waves: status and point of every element (the
    G1 form of this test over the fixtures once each is test_gpu_msm.py::test_g1_deserialize_rejects_mixed_batch)"""
    F, aff, unit = _curve(o, group)
    batch = _mixed_batch(group)
    blob = b"".join(bytes.fromhex(c["bytes"]) for c in batch)
    pts, st = ctx.deserialize_batch(group, blob, True, True)
    assert list(st) == [c["status"] for c in batch]
    for k, c in enumerate(batch):
        assert pts[aff * k:aff * (k + 1)] == (bytes.fromhex(c["affine"]) if c["status"] == 0 else bytes(aff)), (k, c["name"])


@pytest.mark.parametrize("group", GROUPS)
def test_check_batch_on_the_unvalidated_decode(ctx, o, group):
    """the same batch decoded WITHOUT validation, then Valid::batch_check on the points: the oracle's statuses (a malformed encoding
    decodes to the all-zero point, which is infinity and valid); with the off-curve fixture appended for status 2"""
    F, aff, unit = _curve(o, group)
    deser = o.g1_deserialize if group == "g1" else o.g2_deserialize
    batch = _mixed_batch(group)
    blob = b"".join(bytes.fromhex(c["bytes"]) for c in batch)
    pts, st = ctx.deserialize_batch(group, blob, True, False)
    want_st, want_pts, want_chk = [], [], []
    for c in batch:
        pt, s = deser(bytes.fromhex(c["bytes"]), True, False)
        want_st.append(s)
        want_pts.append(o.affine_to_bytes(F, pt) if s == 0 else bytes(aff))
        want_chk.append(deser(bytes.fromhex(c["bytes"]), True, True)[1] if s == 0 else 0)
    assert list(st) == want_st and pts == b"".join(want_pts)
    assert set(want_st) == {0, 1} and set(want_chk) == {0, 3}
    off = [c for c in _golden()[f"{group}_encoding"] if c["name"] == "not_on_curve_uncompressed_unvalidated"]
    assert len(off) == 1 and off[0]["status"] == 0
    points = pts[:aff * 5] + bytes.fromhex(off[0]["affine"]) + pts[aff * 5:] + bytes.fromhex(off[0]["affine"])
    want = want_chk[:5] + [2] + want_chk[5:] + [2]
    assert list(ctx.check_batch(group, points)) == want


@pytest.mark.parametrize("group", GROUPS)
def test_rejected_compressed_set_leaves_the_installed_one(pkg, co, o, group):
    """set_bases_from_compressed(validate) over a batch with rejects: MI_E_INVALID, n_rejected = the oracle's count, nothing installed —
    an MSM over the set installed before still equals the closed form"""
    F, aff, unit = _curve(o, group)
    n = 400
    bases = co.gen_bases(group, 0xC0DEC, n, 4)
    sc = co.gen_scalars(0xC0DED, n)
    want = co.dlog_expected(group, sc, 0xC0DEC, n)
    batch = _mixed_batch(group)
    blob = b"".join(bytes.fromhex(c["bytes"]) for c in batch)
    rejects = sum(1 for c in batch if c["status"] != 0)
    assert 0 < rejects < len(batch)
    with pkg.Context([0]) as c:
        c.set_bases(group, bases, n)
        assert co.to_affine(group, c.msm(group, None, sc, n, 0)) == want
        rej = C.c_size_t(0)
        rc = getattr(c._L, f"mi_msm_{group}_set_bases_from_compressed")(c._h, blob, len(batch), 1, 1, C.byref(rej))
        assert rc == -1 and rej.value == rejects                                  # MI_E_INVALID
        assert c.set_bases_from_compressed(group, blob, len(batch), True, True) == rejects
        assert co.to_affine(group, c.msm(group, None, sc, n, 0)) == want
        # unvalidated, only the malformed encodings are rejected
        malformed = sum(1 for x in batch if x["status"] == 1)
        assert c.set_bases_from_compressed(group, blob, len(batch), True, False) == malformed
        assert co.to_affine(group, c.msm(group, None, sc, n, 0)) == want
