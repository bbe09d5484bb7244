"""The closed-form transforms of tests/ntt_edge_cases.py against the oracle, before anything runs on a GPU: a convention slip (index
order, bit reversal, the 1/n, the sign of the exponent) shows here. oracle.ntt.Domain at 2^1, 2^2, 2^3, 2^5, 2^8 on the three scalar
fields; oracle.cbridge.ntt (the C restatement) at 2^12 and 2^14, so the device tests may take it as the oracle at the larger sizes."""
import numpy as np
import pytest

from oracle import cbridge, ntt
from tests import helpers as H
from tests import ntt_edge_cases as E

CURVES = ["bn254", "bls12_381", "bls12_377"]


def _gen(F, logn):
    return ntt.roots_of_unity(F)[1][logn]


@pytest.mark.parametrize("curve", CURVES)
def test_saturated_word_is_a_canonical_residue_with_all_ones_limbs(curve):
    F = H.FR[curve]
    assert E.SATURATED_WORD < F.p
    assert all((E.SATURATED_WORD >> (29 * i)) & ((1 << 29) - 1) == (1 << 29) - 1 for i in range(8))
    assert F.to_mont(E.saturated_value(F)) == E.SATURATED_WORD


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("logn", [1, 2, 3, 5, 8])
def test_closed_forms_equal_the_oracle_domain(curve, logn):
    F = H.FR[curve]
    g = _gen(F, logn)
    dom = ntt.Domain(F, 1 << logn, g)
    cases = E.families(F, logn, g)
    fams = {c.family for c in cases}
    assert fams == {"zeros", "const", "char", "delta", "edge", "sat", "tone"}
    for c in cases:
        assert all(0 <= x < F.p for x in c.inv_in + c.fwd_in), c.name
        want_i, want_f = dom.ifft_in_to_out(c.inv_in), dom.fft_out_to_in(c.fwd_in)
        if c.inv_out is None:
            assert c.family in ("edge", "sat") and c.fwd_out is None
            continue
        assert c.inv_out == want_i, (c.name, "ifft_in_to_out")
        assert c.fwd_out == want_f, (c.name, "fft_out_to_in")
        # the natural-order entry points are the same transforms behind a bit reversal
        assert dom.fft(ntt.bit_reverse(c.fwd_in)) == c.fwd_out, (c.name, "fft")
        assert dom.ifft(c.inv_in) == ntt.bit_reverse(c.inv_out), (c.name, "ifft")
    for ca, cb in E.share_pairs(cases):
        assert ca.family != cb.family


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("logn", [12, 14])
def test_c_restatement_equals_the_closed_forms(curve, logn):
    F = H.FR[curve]
    cid = H.CURVE_IDS[curve]
    g = _gen(F, logn)
    pg = H.pack(F, [g])
    for c in E.families(F, logn, g):
        if c.inv_out is None:
            continue
        got_i = cbridge.ntt(cid, H.pack(F, c.inv_in), logn, pg, dif=True)
        got_f = cbridge.ntt(cid, H.pack(F, c.fwd_in), logn, pg, dif=False)
        assert np.array_equal(got_i, H.pack(F, c.inv_out)), (c.name, "ifft_in_to_out")
        assert np.array_equal(got_f, H.pack(F, c.fwd_out)), (c.name, "fft_out_to_in")


@pytest.mark.parametrize("curve", CURVES)
def test_c_restatement_equals_the_oracle_domain_on_the_mixes(curve):
    """the two families without a closed form, at a size both oracles reach"""
    F = H.FR[curve]
    logn = 8
    g = _gen(F, logn)
    dom = ntt.Domain(F, 1 << logn, g)
    for c in (E.edge_mix_case(F, logn, 7), E.saturated_mix_case(F, logn)):
        for dif, want in ((True, dom.ifft_in_to_out(c.inv_in)), (False, dom.fft_out_to_in(c.fwd_in))):
            got = cbridge.ntt(H.CURVE_IDS[curve], H.pack(F, c.inv_in), logn, H.pack(F, [g]), dif=dif)
            assert H.unpack(F, got) == want, (c.name, dif)


def test_h_reference_forms_agree():
    """h_rep3 on shares (a, 0), (b, 0) with zero masks is h_plain(a, b); h of b = 0 is zero; h of two characters j1 + j2 = n
    (product = the constant c1 c2) is checked against the polynomial identity on the coset directly."""
    F = H.FR["bn254"]
    logn = 4
    n = 1 << logn
    p = F.p
    g = _gen(F, logn)
    shift = ntt.roots_of_unity(F)[1][logn + 1]
    dom = ntt.Domain(F, n, g)
    r = H.rng(3)
    a, b = H.rand_elems(F, n, r), H.rand_elems(F, n, r)
    ce = E.make_coset_eval(F, dom, shift)
    want = E.h_plain(F, ce, a, b)
    assert E.h_rep3(F, ce, [(x, 0) for x in a], [(x, 0) for x in b], [0] * n, [0] * n) == want
    assert E.h_plain(F, ce, a, [0] * n) == [0] * n
    # a = evaluations of c1 X^j1, b = of c2 X^j2 on the domain: on the coset point s g^k, a b - (ab mod X^n - 1) = c1 c2 (s^n - 1)
    j1, c1, c2 = 3, p - 1, E.saturated_value(F)
    ca = E.character_case(F, logn, g, j1, "", c1).inv_in
    cb = E.character_case(F, logn, g, n - j1, "", c2).inv_in
    assert E.h_plain(F, ce, ca, cb) == [c1 * c2 * (pow(shift, n, p) - 1) % p] * n


@pytest.mark.parametrize("curve", CURVES)
def test_c_restatement_coset_evaluation_equals_the_oracle(curve):
    """the expectation of the device test of the fused pair kernel (C restatement: transform, coset table, product, transform) is the
    oracle's make_coset_eval, on a character (sparse coefficients) and on the edge mix"""
    F = H.FR[curve]
    cid = H.CURVE_IDS[curve]
    logn = 6
    n = 1 << logn
    g = _gen(F, logn)
    shift = ntt.roots_of_unity(F)[1][logn + 1]
    ce = E.make_coset_eval(F, ntt.Domain(F, n, g), shift)
    pg, ps = H.pack(F, [g]), H.pack(F, [shift])
    table = cbridge.coset_table(cid, ps, logn)
    assert H.unpack(F, table) == ntt.bit_reversed_coset_table(F, shift, n)
    for c in (E.character_case(F, logn, g, n - 1, "sat", E.saturated_value(F)), E.edge_mix_case(F, logn, 5)):
        coeffs = cbridge.ntt(cid, H.pack(F, c.inv_in), logn, pg, dif=True)
        got = cbridge.ntt(cid, cbridge.vec_mul(cid, coeffs, table), logn, pg, dif=False)
        assert H.unpack(F, got) == ce(c.inv_in), c.name
