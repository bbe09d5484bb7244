"""CPU tests of the division by (X - r) (csrc/field_scan.hip: csh_poly_div_linear): the C boundary without a device, and the arithmetic
itself -- lane runs, the weighted-sum levels across lanes and waves with their folds, the one-multiplication-per-element output chain --
run on the host from the same templates the gfx950 kernels instantiate, with the limb-bound contract checks of selftest.hip on (a
violated bound aborts the process, so "the checks are silent" is the test finishing at all)."""
import ctypes as C
import re

import numpy as np
import pytest

from tests import helpers as H

CURVES = ["bn254", "bls12_381", "bls12_377"]
CITES = ["polynomial.rs:183", "shared_polynomial.rs:92-140", "co-noir-common/src/lib.rs:43-47", "68-73", "co_shplemini_prover.rs:661-737",
         "shplemini_prover.rs:594", "co-plonk/src/round5.rs:78-91", ":255", ":274"]
ENTRY_POINTS = {"csh_poly_div_linear_dev": CITES, "csh_poly_div_linear": CITES}
NO_DEVICE, INVALID = -2, -1


def reference_recurrence(p, coeffs, root):
    """The reference's loop as the reference writes it (polynomial.rs:183 ff.): b_i = (a_i - b_(i-1)) (-r)^-1, all n of them -- the
    quotient is b[:-1], the element factor_roots pops is b[-1]."""
    root_inverse = pow(-root % p, -1, p)
    out, temp = [], 0
    for a in coeffs:
        temp = (a - temp) % p
        temp = temp * root_inverse % p
        out.append(temp)
    return out


def test_header_declares_the_entry_points_with_their_reference_lines(hip):
    """Both prototypes are in include/cosnarks_hip.h, and the comment right above the pair cites the reference lines it replaces and
    says that the strided zerofier is not built."""
    from cosnarks_amd import bindings
    txt = open(bindings.header_path()).read()
    declared = bindings.declared_symbols()
    L = hip.lib()
    for name, cites in ENTRY_POINTS.items():
        assert name in declared and hasattr(L, name), name
        at = txt.index("int %s(" % name)
        comment = txt[txt.rindex("/*", 0, at):at]
        for c in cites:
            assert c in comment, (name, c)
        assert re.search(r"NOT built: div_by_zerofier with a stride", comment)


def _args():
    a = np.zeros(8 * 4, dtype=np.uint64)
    out = np.zeros(8 * 4, dtype=np.uint64)
    rem = np.zeros(2 * 4, dtype=np.uint64)
    root = np.ones(4, dtype=np.uint64)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    return a, out, rem, root, p


def test_argument_checks_come_before_the_device(hip):
    """An unknown curve or Grumpkin, ncomp outside {1, 2}, NULL in / out with n > 1, NULL root, root = 0, n above 2^28 and accumulate
    with out == in answer CSH_ERR_INVALID on any machine."""
    L = hip.lib()
    a, out, rem, root, p = _args()
    zero = np.zeros(4, dtype=np.uint64)
    n, big = C.c_size_t(4), C.c_size_t((1 << 28) + 1)
    dev = lambda f, i, cnt, ncomp, rt, acc, o: L.csh_poly_div_linear_dev(f, i, cnt, ncomp, rt, None, None, acc, o, p(rem), None)
    host = lambda f, i, cnt, ncomp, rt, o: L.csh_poly_div_linear(f, i, cnt, ncomp, rt, None, o, p(rem))
    for bad_curve in (2, 7):   # Grumpkin has no scalar-field entry points; 7 is no curve
        assert dev(bad_curve, p(a), n, 1, p(root), 0, p(out)) == INVALID
        assert host(bad_curve, p(a), n, 1, p(root), p(out)) == INVALID
    for f in (0, 1, 3):
        for ncomp in (0, 3):
            assert dev(f, p(a), C.c_size_t(2), ncomp, p(root), 0, p(out)) == INVALID
            assert host(f, p(a), C.c_size_t(2), ncomp, p(root), p(out)) == INVALID
        assert b"ncomp" in L.csh_last_error()
        assert dev(f, None, n, 1, p(root), 0, p(out)) == INVALID
        assert dev(f, p(a), n, 1, p(root), 0, None) == INVALID
        assert host(f, None, n, 1, p(root), p(out)) == INVALID
        assert host(f, p(a), n, 1, p(root), None) == INVALID
        assert dev(f, p(a), n, 1, None, 0, p(out)) == INVALID
        assert host(f, p(a), n, 1, None, p(out)) == INVALID
        assert dev(f, p(a), n, 2, p(zero), 0, p(out)) == INVALID
        assert b"shift" in L.csh_last_error()
        assert host(f, p(a), n, 1, p(zero), p(out)) == INVALID
        assert b"shift" in L.csh_last_error()
        assert dev(f, p(a), big, 1, p(root), 0, p(out)) == INVALID
        assert host(f, p(a), big, 1, p(root), p(out)) == INVALID
        assert b"2^28" in L.csh_last_error()
        assert dev(f, p(a), n, 1, p(root), 1, p(a)) == INVALID
        assert b"accumulate" in L.csh_last_error()


def test_no_device_no_result(hip):
    """Without a device every valid call, n = 0 included, fails with the no-device error: there is no CPU path."""
    if hip.have_device():
        pytest.skip("a HIP device is present")
    L = hip.lib()
    a, out, rem, root, p = _args()
    for f in (0, 1, 3):
        for n in (C.c_size_t(4), C.c_size_t(1), C.c_size_t(0)):
            for rc in (L.csh_poly_div_linear_dev(f, p(a), n, 1, p(root), None, None, 0, p(out), p(rem), None),
                       L.csh_poly_div_linear_dev(f, p(a), n, 2, p(root), p(rem), p(root), 1, p(out), None, None),
                       L.csh_poly_div_linear(f, p(a), n, 2, p(root), None, p(out), p(rem)),
                       L.csh_poly_div_linear(f, p(a), n, 1, p(root), p(rem), p(out), None)):
                assert rc == NO_DEVICE
                assert re.search(b"no HIP device|no CPU fallback", L.csh_last_error())
    with pytest.raises(hip.CoSnarksHipError, match="no HIP device|no CPU fallback"):
        hip.poly_div_linear(hip.BN254, a, root)


def _divlin_host(hip, curve, vals, ncomp, run, root, sub0=None):
    """vals: n x ncomp integers, interleaved -> all n x ncomp values b (interleaved alike) from csh_selftest_divlin_host."""
    F = H.FR[curve]
    n = len(vals) // ncomp
    a = H.pack(F, vals)
    out = np.zeros(4 * len(vals), dtype=np.uint64)
    rt = H.pack(F, [root])
    s0 = H.pack(F, sub0) if sub0 is not None else None
    p = lambda x: x.ctypes.data_as(C.c_void_p) if x is not None else None
    rc = hip.lib().csh_selftest_divlin_host(H.CURVE_IDS[curve], p(a), C.c_size_t(n), C.c_uint32(ncomp), run, p(rt), p(s0), p(out))
    assert rc == 0
    H.assert_canonical(F, out)
    return H.unpack(F, out)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("ncomp", [1, 2])
@pytest.mark.parametrize("run", [1, 4, 8])
def test_lane_runs_and_levels_known_answers(hip, curve, ncomp, run):
    """The kernels' arithmetic lane after lane on the host, bound checks on: edge values followed by random ones (more than one wave of
    lanes at run 1), the top of the field against the roots whose powers are +-1, ones, and a single element."""
    F = H.FR[curve]
    r = H.rng(500 + run)
    root = r.randrange(1, F.p)
    edge = [v % F.p for v in H.edge_elems(F)]
    cases = [(edge * ncomp + H.rand_elems(F, 75 * ncomp, r), root), ([F.p - 1] * (37 * ncomp), F.p - 1), ([F.p - 1] * (37 * ncomp), 1),
             ([1] * (19 * ncomp), root), ([5] * ncomp, root)]
    for vals, rt in cases:
        want = [None] * len(vals)
        for c in range(ncomp):
            want[c::ncomp] = reference_recurrence(F.p, vals[c::ncomp], rt)
        assert _divlin_host(hip, curve, vals, ncomp, run, rt) == want, (curve, ncomp, run, len(vals), hex(rt))
    # sub0: the value every call site takes off coefficient 0 first
    vals, sub = cases[0][0], [F.p - 1, 3][:ncomp]
    shifted = list(vals)
    for c in range(ncomp):
        shifted[c] = (vals[c] - sub[c]) % F.p
    want = [None] * len(vals)
    for c in range(ncomp):
        want[c::ncomp] = reference_recurrence(F.p, shifted[c::ncomp], root)
    assert _divlin_host(hip, curve, vals, ncomp, run, root, sub0=sub) == want
    assert hip.lib().csh_selftest_divlin_host(H.CURVE_IDS[curve], None, C.c_size_t(0), 1, 3, None, None, None) == INVALID
