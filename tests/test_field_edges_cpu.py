"""The device field arithmetic at the limb and value bounds of its documented contracts, on the HOST build of the same headers
(csrc/fp28.cuh, ec.cuh compiled with g++ through tests/host/fp28_host_check.cpp): every one-lane op of the raw-limb table
(csrc/field_test_ops.cuh) on the vectors of tests/field_vectors_util.py, checked against Python integers.  Runs without a GPU and so
proves the generator, its legality assertions and the integer reference that tests/test_gpu_field_edges.py uses on the device."""
import pytest

import tests.field_vectors_util as fv

HOST_FAMILIES = ["fp_mul", "fp_linear", "fp_reduce", "fp2_lane", "madd", "conv"]


def test_op_table_matches_the_generator():
    ops = fv.host_ops()
    assert sorted(o[0] for o in ops) == sorted(fv.OPS), set(o[0] for o in ops) ^ set(fv.OPS)
    host = {o[0] for o in ops if o[3] == 0}
    assert {fv.OPS[n]["family"] for n in host} == set(HOST_FAMILIES)
    assert {n for n in fv.OPS if fv.OPS[n]["family"] in ("coop", "kara", "line") or n == "madd_g2"} == set(fv.OPS) - host   # device only


def test_every_vector_is_inside_its_documented_contract():
    for name in fv.OPS:
        vecs = fv.vectors(name)      # asserts legality of each
        tags = {v.tag.split(":")[0].split("/")[0] for v in vecs}
        assert "maxcol" in tags or fv.OPS[name]["family"] in ("fp_reduce", "coop", "fp2_lane"), (name, tags)


@pytest.mark.parametrize("family", HOST_FAMILIES)
def test_host_build_at_the_edges(family):
    ops = {o[0]: o for o in fv.host_ops()}
    names = [n for n in fv.OPS if fv.OPS[n]["family"] == family and ops[n][3] == 0]
    assert names
    for name in names:
        fv.check(name, fv.unpack(fv.host_run(name), ops[name][2]))


def test_column_model_of_the_device_only_accumulators():
    """The Karatsuba / four-product accumulators have no host build; their vectors, legality and reference are proved here against a
    restatement of the column arithmetic (signed 64-bit columns included: every column must stay inside +-2^63)."""
    for name, model in fv.MODELS.items():
        res = [([r0, r1], 0) for r0, r1 in (model(v) for v in fv.vectors(name))]
        fv.check(name, res)
        assert fv.peak_fraction(name) < 1.0, name
    # the Karatsuba contract is the operand bounds AND sum a1' g1 <= 144 p^2 (comment above KaraCols): with every operand at its bound
    # over four terms V1 = 192 p^2 exceeds the bias p 2^388 and the reduction's input is negative; the generator refuses such a vector
    corner = fv.kara_vec("beyond the bias", [((fv.ZERO, fv.maxlow(8 * fv.P + 1), fv.ZERO, fv.maxlow(6 * fv.P + 1)), 0)] * 4)
    with pytest.raises(AssertionError):
        fv.OPS["kara"]["legal"](corner)


def test_the_three_forms_of_a_multiplier_agree_bit_for_bit():
    """fp28.cuh: "two forms with the same multiply-adds and the same column sums (bit-identical results)" """
    for base in ("fp_mul", "fp_sqr", "fp_mul2add"):
        assert fv.host_run(base) == fv.host_run(base + "_os") == fv.host_run(base + "_call"), base
    for op in ("mul", "sqr", "sqr_sub12sqr", "mul_b3", "is_zero_2p"):      # Fp2: the shared-call and the inlined bodies
        assert fv.host_run("fp2c_" + op) == fv.host_run("fp2i_" + op), op


def test_column_magnitudes_reached():
    """How close to the 64-bit limit the vectors drive a column (a model of the column arithmetic, reported in the pull request): the
    multiplier vectors must reach what the documented limb bounds allow: 13 low limbs of 2^29.5 give a column of 13 * 2^59 = 0.406 * 2^64."""
    assert fv.peak_fraction("fp_mul") > 0.406
    assert fv.peak_fraction("kara") > 0.5 and fv.peak_fraction("acc4") > 0.6
