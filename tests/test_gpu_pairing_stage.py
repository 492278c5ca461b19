"""The production kernels of the pairing row, one stage at a time, ON THE DEVICE, on inputs the test constructs at the edges of the
contracts their comments state (tests/pairing_stage_util.py, tests/field_vectors_util.py; tests/test_pairing_stage_cpu.py proves the
vectors and the integer reference without a GPU):
  coop_line_dbl / coop_line_add   ops of the raw-limb field table, in a kernel of k_miller_lines2's shape (tests/test_gpu_field_edges.py
                                  checks them against the integer formulas; here: against the generic Tower<PF2> on the host)
  k_miller_accumulate             whole line buffers in the production layout, m pairs per accumulator
  k_fp12_prod                     one tree level, the unpaired last value limb for limb
  k_fp12_to_raw                   canonical words
Residue-exact or bit-exact everywhere; one small launch per case."""
import pytest

import tests.field_vectors_util as fv
import tests.pairing_stage_util as ps

pytestmark = pytest.mark.gpu


def test_line_steps_agree_with_the_generic_tower_on_the_host(tctx):
    """coop_line_dbl / coop_line_add are re-ordered copies of pairing::Tower::line_dbl / line_add: equal residues on every vector
    (an element with the sink's `inf` set stores (1, 0, 0) instead of the line: its T is compared, its line is checked limb for limb)"""
    table = tctx.test_field_ops()
    index = {o[0]: i for i, o in enumerate(table)}
    for name in ("line_dbl", "line_add"):
        vecs = fv.vectors(name)
        _, nin, nout, kind = table[index[name]]
        assert (nin, nout, kind) == (12 if name == "line_add" else 8, 12, 3)
        dev = fv.unpack(tctx.test_field_op(index[name], fv.pack(vecs, nin), len(vecs)), nout)
        host = ps.host_line_results(name)
        fv.check(name, dev)
        for v, (sd, _), (sh, _) in zip(vecs, dev, host):
            first = 6 if v.aux & 1 else 0
            assert [fv.val(x) % fv.P for x in sd[first:]] == [fv.val(x) % fv.P for x in sh[first:]], (name, v.tag)
            if v.aux & 1:
                assert sd[:6] == [fv.C["ONE"]] + [fv.ZERO] * 5, (name, v.tag)


@pytest.mark.parametrize("m", [1, 2, 7, 8])
def test_accumulate_kernel_on_constructed_line_buffers(tctx, m):
    """k_miller_accumulate: n in {1, m, m + 1, 10 m, 10 m + 1} (a ragged last group, a full wave, a second wave whose nine idle groups
    shadow the one live group), lines at the top of the contract, infinity lines, zero coefficients in both spellings, an all-zero line"""
    for mm, n in ps.ACC_SHAPES:
        if mm != m:
            continue
        _, data, _, _ = ps.acc_case(m, n)
        out = tctx.test_pairing_stage("accumulate", data, n, m)
        ps.check_accumulate(m, n, out)


def test_tree_level_on_constructed_operands(tctx):
    """k_fp12_prod: out[g] = in[2g] in[2g+1]; zero in both spellings, one, p - 1, 2p - 1, sparse values, the corner of "a <= 4p";
    an unpaired last value comes back limb for limb"""
    for n in ps.PROD_SIZES:
        out = tctx.test_pairing_stage("prod", ps.pack_fp12(ps.prod_case(n)), n)
        ps.check_prod(n, out)


def test_to_raw_is_canonical(tctx):
    """k_fp12_to_raw: every word group is the canonical integer x 2^384 mod p, below p, for inputs up to the top of fp_to_blst's contract"""
    vals = ps.to_raw_case()
    for n in (1, 64):
        ps.check_to_raw(vals[:n], tctx.test_pairing_stage("to_raw", ps.pack_fp12(vals[:n]), n))


def test_stage_hook_refuses_a_buffer_of_the_wrong_size(pkg, tctx):
    _, data, _, _ = ps.acc_case(2, 3)
    for bad in ((data[:-4], 3, 2), (data, 21, 2), (data, 3, 0)):
        with pytest.raises(pkg.MsmError):
            tctx.test_pairing_stage("accumulate", *bad)
    with pytest.raises(pkg.MsmError):
        tctx.test_pairing_stage("to_raw", ps.pack_fp12(ps.prod_case(41)) * 2, 82)
