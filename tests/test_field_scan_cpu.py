"""CPU tests of the field scans (csrc/field_scan.hip: running product, batch inverse, polynomial evaluation): the C boundary without a
device, the tune keys, and the arithmetic itself -- the windowed inversion of the spine and the scale bookkeeping of the lane runs --
run on the host from the same templates the gfx950 kernels instantiate, with the limb-bound contract checks of selftest.hip on."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import fields as fl
from tests import helpers as H

CURVES = ["bn254", "bls12_381", "bls12_377"]
ENTRY_POINTS = {
    "csh_vec_prefix_prod_dev": ["round2.rs:164-165", "mpc/rep3.rs:211-213"],
    "csh_vec_prefix_prod": ["round2.rs:164-165", "mpc/rep3.rs:211-213"],
    "csh_vec_batch_inverse_dev": ["co-noir-common/src/mpc/rep3.rs:208-257", "rep3/arithmetic.rs:233-246", "rep3/detail.rs:487", "plain.rs:127-140"],
    "csh_vec_batch_inverse": ["co-noir-common/src/mpc/rep3.rs:208-257", "rep3/arithmetic.rs:233-246", "rep3/detail.rs:487", "plain.rs:127-140"],
    "csh_eval_poly_dev": ["round4.rs:126-132", "co_shplemini_prover.rs:382-444", "rep3/poly.rs:39-68"],
    "csh_eval_poly": ["round4.rs:126-132", "co_shplemini_prover.rs:382-444", "rep3/poly.rs:39-68"],
}
NO_DEVICE, INVALID = -2, -1


def test_header_declares_the_entry_points_with_their_reference_lines(hip):
    """Each of the six prototypes is in include/cosnarks_hip.h, and the comment right above its pair cites the reference lines it replaces."""
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


def _args(hip):
    a = np.zeros(8 * 4, dtype=np.uint64)
    out = np.zeros(8 * 4, dtype=np.uint64)
    zc = C.c_size_t(0)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    return a, out, zc, p


def test_argument_checks_come_before_the_device(hip):
    """ncomp outside {1, 2}, NULL with n > 0, an unknown curve and n above 2^28 answer CSH_ERR_INVALID on any machine."""
    L = hip.lib()
    a, out, zc, p = _args(hip)
    n, st = C.c_size_t(8), None
    pt = np.ones(4, dtype=np.uint64)
    big = C.c_size_t((1 << 28) + 1)
    for bad_curve in (2, 7):   # Grumpkin has no scalar-field entry points; 7 is no curve
        assert L.csh_vec_prefix_prod_dev(bad_curve, p(a), p(out), n, st) == INVALID
        assert L.csh_vec_prefix_prod(bad_curve, p(a), p(out), n) == INVALID
        assert L.csh_vec_batch_inverse_dev(bad_curve, p(a), p(out), n, None, st) == INVALID
        assert L.csh_vec_batch_inverse(bad_curve, p(a), p(out), n, C.byref(zc)) == INVALID
        assert L.csh_eval_poly_dev(bad_curve, p(a), n, 1, p(pt), p(out), st) == INVALID
        assert L.csh_eval_poly(bad_curve, p(a), n, 1, p(pt), p(out)) == INVALID
    for f in (0, 1, 3):
        assert L.csh_vec_prefix_prod_dev(f, None, p(out), n, st) == INVALID
        assert L.csh_vec_prefix_prod_dev(f, p(a), None, n, st) == INVALID
        assert L.csh_vec_prefix_prod(f, None, p(out), n) == INVALID
        assert L.csh_vec_prefix_prod(f, p(a), p(out), big) == INVALID
        assert L.csh_vec_batch_inverse_dev(f, None, p(out), n, None, st) == INVALID
        assert L.csh_vec_batch_inverse(f, p(a), None, n, None) == INVALID
        assert L.csh_vec_batch_inverse_dev(f, p(a), p(out), big, None, st) == INVALID
        for ncomp in (0, 3):
            assert L.csh_eval_poly_dev(f, p(a), C.c_size_t(2), ncomp, p(pt), p(out), st) == INVALID
            assert L.csh_eval_poly(f, p(a), C.c_size_t(2), ncomp, p(pt), p(out)) == INVALID
        assert L.csh_eval_poly_dev(f, None, n, 1, p(pt), p(out), st) == INVALID
        assert L.csh_eval_poly(f, p(a), n, 1, None, p(out)) == INVALID
        assert L.csh_eval_poly(f, p(a), n, 1, p(pt), None) == INVALID
        assert L.csh_eval_poly(f, p(a), big, 1, p(pt), p(out)) == INVALID
    assert b"ncomp" in L.csh_last_error() or b"2^28" in L.csh_last_error()


def test_no_device_no_result(hip):
    """Without a device every entry point, n = 0 included, fails with the no-device error: there is no CPU path."""
    if hip.have_device():
        pytest.skip("a HIP device is present")
    L = hip.lib()
    a, out, zc, p = _args(hip)
    pt = np.ones(4, dtype=np.uint64)
    for f in (0, 1, 3):
        for n in (C.c_size_t(8), C.c_size_t(0)):
            for rc in (L.csh_vec_prefix_prod_dev(f, p(a), p(out), n, None), L.csh_vec_prefix_prod(f, p(a), p(out), n),
                       L.csh_vec_batch_inverse_dev(f, p(a), p(out), n, None, None), L.csh_vec_batch_inverse(f, p(a), p(out), n, C.byref(zc)),
                       L.csh_eval_poly_dev(f, p(a), n, 2, p(pt), p(out), None), L.csh_eval_poly(f, p(a), n, 1, p(pt), p(out))):
                assert rc == NO_DEVICE
                assert re.search(b"no HIP device|no CPU fallback", L.csh_last_error())
    for call in (lambda: hip.vec_prefix_prod(hip.BN254, a), lambda: hip.vec_batch_inverse(hip.BN254, a), lambda: hip.eval_poly(hip.BN254, a, pt)):
        with pytest.raises(hip.CoSnarksHipError, match="no HIP device|no CPU fallback"):
            call()


def test_tune_keys_exist_validate_and_restore(hip):
    B = hip.bindings
    defaults = {"scan_lane_run": 8, "scan_tile_lanes": 256, "scan_spine_step": 1024}
    good = {"scan_lane_run": [4, 8], "scan_tile_lanes": [64, 128, 256], "scan_spine_step": [64, 128, 256, 512, 1024]}
    bad = {"scan_lane_run": [0, 1, 2, 3, 6, 16, -4], "scan_tile_lanes": [0, 32, 96, 512, 1024, -64], "scan_spine_step": [0, 32, 100, 2048, -1]}
    for key, dflt in defaults.items():
        assert B.tune_get(key) == dflt
        for v in bad[key]:
            with pytest.raises(hip.CoSnarksHipError, match="out of range"):
                B.tune_set(key, v)
            assert B.tune_get(key) == dflt
        for v in good[key]:
            with hip.tuned(**{key: v}):
                assert B.tune_get(key) == v
            assert B.tune_get(key) == dflt


def _scan_host(hip, curve, op, vals, run):
    F = H.FR[curve]
    n = len(vals)
    a = H.pack(F, vals) if n else np.zeros(4, dtype=np.uint64)
    out = np.zeros(4 * max(n, 1), dtype=np.uint64)
    rc = hip.lib().csh_selftest_scan_host(H.CURVE_IDS[curve], op, a.ctypes.data_as(C.c_void_p), C.c_size_t(n), run, out.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return H.unpack(F, out[:4 * n])


@pytest.mark.parametrize("curve", CURVES)
def test_windowed_inversion_matches_pow(hip, curve):
    """lazy_inv (field_scan.hpp), the one inversion of a batch: a^(p - 2) by fixed 4-bit windows in the lazy field, against pow(a, -1, p).
    0 has no inverse; the exponentiation gives 0, which is what the batch needs (it never sees one: zeros are replaced on load)."""
    F = H.FR[curve]
    vals = [v % F.p for v in H.edge_elems(F)] + [1, F.p - 1, 2] + H.rand_elems(F, 40, H.rng(2024))
    got = _scan_host(hip, curve, 2, vals, 1)
    for v, g in zip(vals, got):
        assert g == (pow(v, -1, F.p) if v else 0), (curve, hex(v))


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("run", [1, 4, 8])
def test_lane_run_scales_known_answers(hip, curve, run):
    """The scale bookkeeping of the kernels, lane after lane on the host: a run's chain scales all but its first operand by 2^5, lane totals
    cross lanes in the lazy Montgomery domain, the carry of the suffix side is back in the arkworks scale. Wrong by one 2^5 anywhere and
    every element after the first run is off by a power of 32. Values at the top of the field drive the products' value bounds."""
    F = H.FR[curve]
    r = H.rng(77 + run)
    for vals in ([v % F.p for v in H.edge_elems(F) if v % F.p] + H.rand_elems(F, 23, r), [F.p - 1] * 37, [1] * 19, [F.p - 2, F.p - 1] * 20, [5]):
        want, acc = [], 1
        for v in vals:
            acc = acc * v % F.p
            want.append(acc)
        assert _scan_host(hip, curve, 0, vals, run) == want
        assert _scan_host(hip, curve, 1, vals, run) == [pow(v, -1, F.p) for v in vals]
    vals = H.rand_elems(F, 30, r)
    for z in (0, 7, 8, 29):
        vals[z] = 0
    assert _scan_host(hip, curve, 1, vals, run) == [pow(v, -1, F.p) if v else 0 for v in vals]
    want, acc = [], 1
    for v in vals:
        acc = acc * v % F.p
        want.append(acc)
    assert _scan_host(hip, curve, 0, vals, run) == want
