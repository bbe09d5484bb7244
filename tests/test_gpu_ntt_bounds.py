"""The limb-bound contract of field29.hpp inside the real NTT kernels, on the device.

csrc/selftest_ntt_dev.hip instantiates the lazy pass kernels of ntt_kernels.hpp a second time -- radix-2, radix-4 and the fused pair,
both directions, three scalar fields -- with CSH_CHECK_BOUNDS_DEVICE: every product checks the limbs of its operands, fold_top() checks
that its quotient estimate stays within the documented |k| <= 64; a violation is counted, never trapped. The entries run a whole
transform through the product's own planning, tables and launch code with those kernels and hand back the data and the record
(violations, largest |limb| or |k|, site = line of field29.hpp). Every launch must return the oracle's transform bit-exactly AND an empty
record, on every family of tests/ntt_edge_cases.py and on one uniformly random vector per kernel form (a record that fills on ordinary
data is thereby told apart from one that fills only at an edge of the range).

Shapes (tune ntt_variant, logn, components), the one-pass, deep-tile and three-pass rows of tests/test_gpu_ntt_edges.py, all three fields:

  variant        logn           ncomp  plan (s0, k, cb)              what it reaches
  1 and 2        1, 2           1, 2   (0,1,0), (0,2,0)              one radix-2 stage / round4_unit alone
  1 and 2        3, 4, 5        1      one pass                      round4_unit, general round4, left-over radix-2 stage
  1 and 2        8              1, 2   (0,8,0) / (0,7,0),(7,1,6)     full default tile; with shares the first strided pass
  0x101, 0x102   11 / 10        1 / 2  (0,11,0) / (0,10,0)           deepest tile: 11 stages between canonicalisations
  0x441, 0x442   14 / 13        1 / 2  three passes                  (0,8,0),(8,3,5),(11,3,5) / (0,7,0),(7,3,4),(10,3,4)
  fused pair     3, 8, 11       1, 2   (0,k,0), k = logn (- 1)       k_ntt_pass_r4<.., PAIR>: DIF rounds, scale table, hand-over, DIT rounds
                                                                     (2^8 and 2^11 shares: one strided pass on either side of the pair)

Nothing here asserts the plan itself."""
import ctypes as C

import numpy as np
import pytest

from oracle import cbridge, ntt
from tests import helpers as H
from tests import ntt_edge_cases as E
from tests.test_gpu_lane_arith import _assert_no_bound_violation, _site

pytestmark = pytest.mark.gpu

CURVES = ["bn254", "bls12_381", "bls12_377"]
_ROWS = [   # (variants, logn, component counts)
    ((1, 2), 1, (1, 2)), ((1, 2), 2, (1, 2)), ((1, 2), 3, (1,)), ((1, 2), 4, (1,)), ((1, 2), 5, (1,)), ((1, 2), 8, (1, 2)),
    ((0x101, 0x102), 11, (1,)), ((0x101, 0x102), 10, (2,)), ((0x441, 0x442), 14, (1,)), ((0x441, 0x442), 13, (2,)),
]


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _err(hip):
    return hip.lib().csh_last_error().decode(errors="replace")


def _gen(F, logn):
    return ntt.roots_of_unity(F)[1][logn]


@pytest.mark.parametrize("curve", CURVES)
def test_ntt_bound_recorder_reports_a_fold_top_quotient_out_of_range(gpu, curve):
    """Positive control of this unit's record and of fold_top()'s site: folding the value R' = 2^261 asks for the quotient R' / p
    (about 170, 70, 440), outside |k| <= 64 -- one lane, one violation, the quotient estimate (exact to +-1) and the line of the
    site. A dead recorder cannot pass; and the record was cleared in between: the same count again."""
    F = H.FR[curve]
    rec = (C.c_uint64 * 3)()
    for _ in range(2):
        assert gpu.lib().csh_selftest_ntt_bound_control_dev(H.CURVE_IDS[curve], rec) == 0, _err(gpu)
        assert rec[0] == 1 and abs(int(rec[1]) - (1 << 261) // F.p) <= 1 and rec[1] > 64, list(rec)
        assert "fold_top(k)" in _site(int(rec[2])), (int(rec[2]), _site(int(rec[2])))


def _checked(gpu, dom, which, vin, ncomp, what):
    """csh_selftest_ntt_dev on a copy of vin -> the transformed array; the record must be empty"""
    d = np.ascontiguousarray(vin, dtype=np.uint64).copy()
    rec = (C.c_uint64 * 3)()
    assert gpu.lib().csh_selftest_ntt_dev(dom.h, which, _ptr(d), C.c_uint32(ncomp), rec) == 0, (_err(gpu), what)
    _assert_no_bound_violation(rec, what)
    return d


@pytest.mark.parametrize("curve,variant,logn,ncomps", [pytest.param(c, v, logn, nc, id="%s-%#x-2^%d" % (c, v, logn))
                                                       for c in CURVES for vs, logn, nc in _ROWS for v in vs])
def test_ntt_kernels_keep_the_limb_bound_contract(gpu, curve, variant, logn, ncomps):
    F = H.FR[curve]
    n = 1 << logn
    pk = E.packed_families(curve, logn)
    dom = gpu.Domain(H.CURVE_IDS[curve], logn, H.pack(F, [_gen(F, logn)]))
    try:
        with gpu.tuned(ntt_variant=variant):
            for ncomp in ncomps:
                for which, entry in ((0, "ifft_in_to_out"), (1, "fft_out_to_in")):
                    if ncomp == 1:
                        for c, io in pk.cases:
                            what = "%s %#x 2^%d %s on '%s'" % (curve, variant, logn, entry, c.name)
                            got = _checked(gpu, dom, which, io[entry][0], 1, what)
                            assert np.array_equal(got.reshape(n, 4), io[entry][1]), what
                    else:
                        for (ca, ioa), (cb, iob) in pk.pairs:
                            what = "%s %#x 2^%d %s on shares {'%s', '%s'}" % (curve, variant, logn, entry, ca.name, cb.name)
                            got = _checked(gpu, dom, which, np.stack([ioa[entry][0], iob[entry][0]], axis=1), 2, what).reshape(n, 2, 4)
                            assert np.array_equal(got[:, 0], ioa[entry][1]) and np.array_equal(got[:, 1], iob[entry][1]), what
    finally:
        dom.free()


def test_checked_ntt_refuses_the_32bit_pass(gpu):
    """the 32-bit pass has no contract and no checked copy: asking for it is an error, not a quiet run of the product kernel"""
    F = H.FR["bn254"]
    dom = gpu.Domain(H.CURVE_IDS["bn254"], 3, H.pack(F, [_gen(F, 3)]))
    d = np.zeros(8 * 4, dtype=np.uint64)
    rec = (C.c_uint64 * 3)()
    try:
        with gpu.tuned(ntt_lazy=0):
            assert gpu.lib().csh_selftest_ntt_dev(dom.h, 0, _ptr(d), C.c_uint32(1), rec) != 0
            assert "kernel table" in _err(gpu)
    finally:
        dom.free()


@pytest.fixture(scope="module")
def coset_evals():
    """Expected outputs of the pair entry per (field, size), computed once with the C restatement (tied to the closed forms and to
    oracle.ntt.Domain by test_ntt_edge_cases_cpu.py): ce(v) = fft_out_to_in(coset_table . ifft_in_to_out(v)) of every family's
    ifft_in_to_out input. -> (shift words, {case name: (n, 4) array})"""
    memo = {}

    def get(curve, logn):
        if (curve, logn) not in memo:
            F = H.FR[curve]
            cid = H.CURVE_IDS[curve]
            pg = H.pack(F, [_gen(F, logn)])
            shift = H.pack(F, [ntt.roots_of_unity(F)[1][logn + 1]])
            table = cbridge.coset_table(cid, shift, logn)
            out = {}
            for c, io in E.packed_families(curve, logn).cases:
                coeffs = cbridge.ntt(cid, io["ifft_in_to_out"][0], logn, pg, dif=True)
                out[c.name] = cbridge.ntt(cid, cbridge.vec_mul(cid, coeffs, table), logn, pg, dif=False).reshape(-1, 4)
            memo[(curve, logn)] = (shift, out)
        return memo[(curve, logn)]
    return get


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("logn", [3, 8, 11])
def test_fused_pair_kernel_keeps_the_limb_bound_contract(gpu, coset_evals, curve, logn):
    """One vector of a witness map (inverse transform, scaled coset table, forward transform) with the fused tile pass forced at every
    size, plain and share vectors, the checked kernels: the oracle's coset evaluation and an empty record."""
    F = H.FR[curve]
    n = 1 << logn
    pk = E.packed_families(curve, logn)
    shift, want = coset_evals(curve, logn)
    dom = gpu.Domain(H.CURVE_IDS[curve], logn, H.pack(F, [_gen(F, logn)]))

    def run(vin, ncomp, what):
        d = np.ascontiguousarray(vin, dtype=np.uint64).copy()
        rec = (C.c_uint64 * 3)()
        assert gpu.lib().csh_selftest_ntt_pair_dev(dom.h, _ptr(shift), _ptr(d), C.c_uint32(ncomp), rec) == 0, (_err(gpu), what)
        _assert_no_bound_violation(rec, what)
        H.assert_canonical(F, d)
        return d
    try:
        with gpu.tuned(ntt_pair=1, ntt_pair_min_log=0):
            for c, io in pk.cases:
                what = "%s 2^%d fused pair on '%s'" % (curve, logn, c.name)
                assert np.array_equal(run(io["ifft_in_to_out"][0], 1, what).reshape(n, 4), want[c.name]), what
            for (ca, ioa), (cb, iob) in pk.pairs:
                what = "%s 2^%d fused pair on shares {'%s', '%s'}" % (curve, logn, ca.name, cb.name)
                got = run(np.stack([ioa["ifft_in_to_out"][0], iob["ifft_in_to_out"][0]], axis=1), 2, what).reshape(n, 2, 4)
                assert np.array_equal(got[:, 0], want[ca.name]) and np.array_equal(got[:, 1], want[cb.name]), what
    finally:
        dom.free()
