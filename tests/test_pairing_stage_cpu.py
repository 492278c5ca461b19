"""The constructed inputs of the pairing-stage tests, proved without a GPU: every vector is inside the contract quoted from the code
under test (asserted when it is generated), the integer reference agrees with the host build of the GENERIC tower
(pairing::Tower<PF2> through tests/host/pairing_host_check.cpp) on the same raw limbs, and the Python layout of the line buffer is
the inverse of a round trip through it.  tests/test_gpu_pairing_stage.py runs the same vectors through the production kernels."""
import tests.field_vectors_util as fv
import tests.pairing_stage_util as ps


def test_line_vectors_are_legal_and_cover_the_classes():
    for name in ("line_dbl", "line_add"):
        vecs = fv.vectors(name)                    # asserts the legality of each
        assert 200 <= len(vecs) <= 500, (name, len(vecs))
        heads = {v.tag.split(":")[0] for v in vecs}
        assert {"maxcol", "value", "spell", "pattern", "random", "zero", "inf"} <= heads, (name, heads)
    assert any(v.tag.startswith("exc:T=+Q") for v in fv.vectors("line_add")) and any(v.tag.startswith("exc:T=-Q") for v in fv.vectors("line_add"))
    # the operand bounds are the quoted ones, not wider: one step beyond each is refused
    v = fv.vectors("line_dbl")[0]
    for k, bad in ((0, fv.exact(6 * fv.P + 1)), (6, fv.exact(2 * fv.P)), (7, fv.exact(2 * fv.P))):
        ins = list(v.ins)
        ins[k] = bad
        try:
            fv.OPS["line_dbl"]["legal"](fv.Vec("beyond", ins))
        except AssertionError:
            continue
        raise AssertionError("operand %d beyond its contract was accepted" % k)


def test_generic_tower_on_the_host_agrees_with_the_integer_formulas_of_the_line_steps():
    """Tower<PF2>::line_dbl / line_add (the originals coop_line_dbl / coop_line_add are copies of) on every vector: residues and the
    output contract of the comment.  Every vector is inside the generic functions' contract too: it is the same comment."""
    for name in ("line_dbl", "line_add"):
        vecs = fv.vectors(name)
        plain = [fv.Vec(v.tag, v.ins, 0) for v in vecs]             # the host has no sink: the `inf` flag does not apply
        res = ps.host_line_results(name)
        bad = []
        for v, (slots, flag) in zip(plain, res):
            outs, _ = fv.OPS[name]["ref"](v)
            try:
                for k, (l, w) in enumerate(zip(slots, outs)):
                    fv.check_out(name, v, k, l, w)
            except AssertionError as e:
                bad.append(str(e))
        assert not bad, "%s: %d of %d vectors fail on the host build, first: %s" % (name, len(bad), len(vecs), bad[0])


def test_line_buffer_layout_round_trip():
    for m, n in ((1, 1), (2, 21), (7, 8), (8, 81)):
        lines, data, _, _ = ps.acc_case(m, n)
        assert len(data) == 4 * ps.line_buffer_words(n, m)
        assert ps.unpack_lines(data, n, m) == [[tuple(tuple(list(c) for c in coeff) for coeff in ln) for ln in per] for per in lines]
        blk = 10 * m
        # the layout function against its definition: blocks of blk pairs, 68 lines each, a pair's line 96 words
        seen = set()
        for pair in range(n):
            for line in range(ps.MILLER_LINES):
                w = ps.line_base_words(pair, blk) + line * blk * 96
                assert w % 96 == 0 and w + 96 <= ps.line_buffer_words(n, m) and w not in seen
                seen.add(w)
                b, i = divmod(pair, blk)
                assert w == ((b * ps.MILLER_LINES + line) * blk + i) * 96
        # the slots of the pairs beyond n stay filled
        if n % blk:
            w = ps.line_base_words(n, blk)
            assert data[4 * w: 4 * w + 8] == b"\xff" * 8


def test_accumulate_buffers_are_legal_and_the_reference_agrees_with_the_generic_tower():
    total = sum(n for _, n in ps.ACC_SHAPES)
    assert 380 <= total <= 420 and len(ps.ACC_SHAPES) == 19       # about 400 pairs over the whole test
    seen = set()
    spent = 0.0
    for m, n in ps.ACC_SHAPES:
        _, _, classes, zero_pair = ps.acc_case(m, n)               # asserts the legality of every line
        seen |= set(classes)
        want, dt = ps.timed(ps.acc_reference, m, n)
        spent += dt
        ps.check_accumulate(m, n, ps.host_accumulate(m, n))        # mul_by_014: "f <= 4p, c0 <= 6p, c1, c4 <= 2p; output < 2p" admits every buffer
    assert seen == set(ps.PAIR_CLASSES)
    print("integer reference of k_miller_accumulate over %d pairs: %.1f s" % (total, spent))
    # the joint condition is part of the contract: a line whose c0.c1, c1.c1, c4.c1 are beyond 36p together is refused
    big = fv.exact(13 * fv.P)
    try:
        ps.legal_line(((fv.ZERO, big), (fv.ZERO, big), (fv.ZERO, big)))
    except AssertionError:
        pass
    else:
        raise AssertionError("a line beyond the contract was accepted")


def test_tree_level_operands_are_legal_and_the_reference_agrees_with_the_generic_tower():
    seen = set()
    for n in ps.PROD_SIZES:
        vals = ps.prod_case(n)                                      # asserts the legality of each
        host = ps.host_prod(n)                                      # mul12: "Inputs <= 4p, output < 2p"
        want = ps.ref_prod(vals)
        for g, limbs in enumerate(ps.unpack_fp12(host)):
            ps.check_fp12("host prod n=%d group %d" % (n, g), limbs, want[g])
        seen |= {tuple(tuple(l) for l in v) for v in vals}
    one = tuple(tuple(l) for l in [ps.ONE] + [fv.ZERO] * 11)
    assert one in seen and tuple(tuple(fv.ZERO) for _ in range(12)) in seen and tuple(tuple(fv.exact(fv.P)) for _ in range(12)) in seen


def test_to_raw_inputs_are_legal_and_reach_the_edges():
    vals = ps.to_raw_case()                                         # asserts the legality of each
    flat = [fv.val(l) for v in vals for l in v]
    assert len(flat) == 768 and {0, 1, fv.P - 1, fv.P, fv.P + 1, 2 * fv.P - 1, fv.TO_BLST_BOUND - 1} <= set(flat)
    # the canonicalisation has work to do: for several inputs the Montgomery product by C_OUT, which is only below 2p, is not below p
    pinv, c_out = pow(fv.P, -1, fv.R), fv.val(fv.C["C_OUT"])
    product = lambda a: (a * c_out + (-a * c_out * pinv) % fv.R * fv.P) // fv.R
    assert sum(product(a) >= fv.P for a in flat) >= 8 and product(flat[0]) < fv.P <= max(product(a) for a in flat[:12])   # also in the first value
    # the checker against the host build of fp_to_blst (the conversion op of the field table) on the same values
    import ctypes

    ops = fv.host_ops()
    idx = [o[0] for o in ops].index("fp_to_blst")
    vecs = [fv.Vec("raw", [l]) for v in vals for l in v]
    out = ctypes.create_string_buffer(64 * len(vecs))
    assert fv.host_lib().h28_field_op(idx, fv.pack(vecs, 1), len(vecs), out) == 0
    raw = b"".join(out.raw[64 * k: 64 * k + 48] for k in range(len(vecs)))
    ps.check_to_raw(vals, raw)


def test_oracles_accept_points_outside_the_subgroups():
    """the inputs of tests/test_gpu_pairing.py::test_points_outside_the_subgroups: on the curves, outside the subgroups where that is
    the point of the pair, accepted by both oracles with equal results, and not one except where the value must be one"""
    from oracle import bls12_381 as o, coracle as co, pairing as pr

    one = pr.fp12_to_bytes(pr.FP12_ONE)
    pairs = ps.unchecked_pairs(o)
    assert len(pairs) == 7
    for name, p1, q2, trivial in pairs:
        assert o.on_curve(o.F1, p1) and o.on_curve(o.F2, q2), name
        assert not (o.g1_in_subgroup(p1) and o.g2_in_subgroup(q2)), name
        assert o.scalar_mul(o.F2, q2, 1 << 64) is not o.INF, name
        want = pr.fp12_to_bytes(pr.pairing(p1, q2))
        assert (want == one) == trivial, name
        assert co.multi_pairing(o.affine_to_bytes(o.F1, p1), o.affine_to_bytes(o.F2, q2), 1) == want, name
