"""The device field arithmetic at the limb and value bounds of its documented contracts, ON THE DEVICE: every op of the raw-limb hook
(mi_test_field_op, csrc/field_test_ops.cuh + field_test_kernels.cuh) on the vectors of tests/field_vectors_util.py — the production
functions of fp28.cuh, ec::Fp2Ops(Inline), the lane-pair CoopF2 / CoopF2A, the Karatsuba and four-product column accumulators of the
pairing kernels, one xyzz_madd step of each accumulate loop — checked against Python integers, against the output contract each comment
promises, and limb for limb against the host build of the same headers where there is one (tests/test_field_edges_cpu.py proves the
vectors and the reference without a GPU).  One small launch per op."""
import pytest

import tests.field_vectors_util as fv

pytestmark = pytest.mark.gpu

FAMILIES = ["fp_mul", "fp_linear", "fp_reduce", "fp2_lane", "coop", "kara", "madd", "conv", "line"]
# every op the hook must accept: none can drop out of the table, the generator or this test unnoticed
OP_NAMES = (["fp_mul", "fp_mul_os", "fp_mul_call", "fp_sqr", "fp_sqr_os", "fp_sqr_call", "fp_mul2add", "fp_mul2add_os", "fp_mul2add_call", "fp_mul4add",
             "fp_add", "fp_add_lazy", "fp_norm"] + [f + str(k) for k in (2, 4, 8, 16, 32, 64) for f in ("fp_sub", "fp_sub_lazy", "fp_neg")] +
            ["fp_sub8_lazy_wide", "fp_mul_small2", "fp_mul_small3", "fp_mul_small12", "fp_mul_small15", "fp_reduce_small", "fp_carry_exact",
             "fp_canon_2p", "fp_is_zero_2p", "fp_is_zero_2p_exact", "fp_is_zero_any"] +
            [v + "_" + f for v in ("fp2c", "fp2i") for f in ("mul", "sqr", "mul2add", "sqr_sub12sqr", "mul_b3", "is_zero_2p")] +
            ["madd_g1", "madd_g2_lane", "fp_from_blst", "fp_to_blst", "coop_mul", "coop_sqr", "coop_sqr_sub12sqr", "coop_mul2add", "coop_mul_b3", "coop_one", "coopa_mul2add",
             "coopa_is_zero_2p", "coopa_limbs_all_zero", "madd_g2", "kara", "kara_pre", "acc4", "line_dbl", "line_add"])


class Device:
    def __init__(self, tctx):
        self.tctx, self.table, self.raw = tctx, tctx.test_field_ops(), {}
        self.index = {o[0]: i for i, o in enumerate(self.table)}

    def run(self, name):
        if name not in self.raw:
            vecs = fv.vectors(name)
            _, nin, nout, _ = self.table[self.index[name]]
            self.raw[name] = self.tctx.test_field_op(self.index[name], fv.pack(vecs, nin), len(vecs))
            assert len(self.raw[name]) == 64 * nout * len(vecs)
        return self.raw[name]

    def results(self, name):
        return fv.unpack(self.run(name), self.table[self.index[name]][2])


@pytest.fixture(scope="module")
def dev(tctx):
    return Device(tctx)


def test_hook_accepts_exactly_the_listed_ops(dev):
    assert [o[0] for o in dev.table] == OP_NAMES
    assert sorted(OP_NAMES) == sorted(fv.OPS)
    assert dev.table == fv.host_ops()                       # one table for the device build and the host build
    assert sorted({fv.OPS[n]["family"] for n in OP_NAMES}) == sorted(FAMILIES)
    with pytest.raises(ValueError):
        dev.tctx.test_field_op(len(OP_NAMES), b"", 1)


@pytest.mark.parametrize("family", FAMILIES)
def test_device_field_ops_at_the_edges(dev, family):
    names = [n for n in OP_NAMES if fv.OPS[n]["family"] == family]
    assert names
    for name in names:
        fv.check(name, dev.results(name))
        if dev.table[dev.index[name]][3] == 0:              # has a host build: the same limbs, not only the same residues
            assert dev.run(name) == fv.host_run(name), name + ": device limbs differ from the host build's"


def test_multiplier_forms_agree_bit_for_bit(dev):
    """fp28.cuh: "two forms with the same multiply-adds and the same column sums (bit-identical results)" """
    for base in ("fp_mul", "fp_sqr", "fp_mul2add"):
        assert dev.run(base) == dev.run(base + "_os") == dev.run(base + "_call"), base
    for f in ("mul", "sqr", "sqr_sub12sqr", "mul_b3", "is_zero_2p"):
        assert dev.run("fp2c_" + f) == dev.run("fp2i_" + f), f


def test_lane_pair_agrees_with_one_lane(dev):
    """The lane-pair Fp2 (DPP partner exchange, lazily negated operands) against the one-lane Fp2 on the same vectors: equal residues and
    verdicts; where both reduce once per component (the fused forms), equal limbs."""
    pairs = [("coop_mul", "fp2i_mul", False), ("coop_sqr", "fp2i_sqr", True), ("coop_sqr_sub12sqr", "fp2i_sqr_sub12sqr", True),
             ("coop_mul2add", "fp2c_mul2add", False), ("coopa_mul2add", "fp2i_mul2add", False), ("coop_mul_b3", "fp2i_mul_b3", False),
             ("madd_g2", "madd_g2_lane", False)]
    for coop, lane, same_limbs in pairs:
        a, b = dev.results(coop), dev.results(lane)
        assert len(a) == len(b) == len(fv.vectors(coop))
        for v, (sa, fa), (sb, fb) in zip(fv.vectors(coop), a, b):
            assert fa == fb, (coop, v.tag)
            assert [fv.val(x) % fv.P for x in sa] == [fv.val(x) % fv.P for x in sb], (coop, v.tag)
            if same_limbs:
                assert sa == sb, (coop, v.tag)
    for (sa, fa), (sb, fb) in zip(dev.results("coopa_is_zero_2p"), dev.results("fp2i_is_zero_2p")):
        assert fa == fb
