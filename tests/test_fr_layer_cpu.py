"""What every scalar-field entry point of vec_ops, field_scan, mle_fold, plonk_quot, sparse and ntt answers to a bad argument, as a table of
literal expectations: the status and a piece of csh_last_error() for Grumpkin, an unknown curve, ncomp 0 and 3, n = 2^28 + 1, a NULL among
the pointers and an in-place call where one is refused. The table was recorded on a machine without a device before the host-side layer
of these units was gathered in csrc/fr_entry.hpp, and holds unchanged after it: a row that reads NO_DEVICE is an entry point that asks for
the device before it looks at that argument (the older vec_ops calls do; the newer units refuse first), and that order is part of the ABI."""
import ctypes as C

import numpy as np
import pytest

OK, INVALID, NO_DEVICE = 0, -1, -2
GRUMPKIN, UNKNOWN = 2, 99
sz, u32 = C.c_size_t, C.c_uint32


class Case:
    """The arguments of one call: valid ones (BN254, 8 elements, one component) with one thing wrong."""

    def __init__(self, name):
        self.f, self.n, self.ncomp, self.null, self.in_place = 0, 8, 1, name == "null", name == "in_place"
        if name == "grumpkin":
            self.f = GRUMPKIN
        elif name == "unknown":
            self.f = UNKNOWN
        elif name in ("ncomp0", "ncomp3"):
            self.ncomp = int(name[-1])
        elif name == "n_big":
            self.n = (1 << 28) + 1


class Bufs:
    """Host memory for every call below: nothing is read or written, a call either is refused or finds no device."""

    def __init__(self):
        z = lambda words: np.zeros(words, dtype=np.uint64)
        self.a, self.b, self.c, self.out, self.out2 = (z(4 * 2 * 64) for _ in range(5))
        self.one = np.ones(4 * 16, dtype=np.uint64)   # a point, a root, challenges, seeds: anything small and non-zero
        self.vecs = [z(4 * 2 * 32) for _ in range(14)]
        self.outs = [z(4 * 2 * 32) for _ in range(10)]
        self.row_ptr = np.zeros(2, dtype=np.uint64)
        self.handle = C.c_void_p(0)
        self.fake_dom = C.c_void_p(self.one.ctypes.data)   # never looked into: refused, or no device, before that


def _p(x):
    return x.ctypes.data_as(C.c_void_p) if x is not None else None


def _ptrs(arrs, hole=None):
    return (C.c_void_p * len(arrs))(*[None if i == hole else a.ctypes.data for i, a in enumerate(arrs)])


def _entry_points(L, B):
    """name -> (call(case), the cases that apply to it). `null` leaves out the pointer each entry names; `in_place` aliases an output with an input."""
    a, b, c, out, one = _p(B.a), _p(B.b), _p(B.c), _p(B.out), _p(B.one)
    no = lambda k, ptr: None if k.null else ptr   # the pointer that the "null" case leaves out
    hole = lambda k, i: i if k.null else None
    CURVE, NCOMP = ("grumpkin", "unknown", "n_big", "null"), ("ncomp0", "ncomp3")
    E = {}
    for dev in (True, False):
        sfx, st = ("_dev", (None,)) if dev else ("", ())
        fn = lambda name, sfx=sfx: getattr(L, name + sfx)
        E["csh_vec_mul" + sfx] = (lambda k, fn=fn, st=st: fn("csh_vec_mul")(k.f, no(k, a), b, out, sz(k.n), *st), CURVE)
        for op in ("csh_vec_add", "csh_vec_sub"):
            E[op + sfx] = (lambda k, fn=fn, st=st, op=op: fn(op)(k.f, no(k, a), b, out, sz(k.n), u32(k.ncomp), *st), CURVE + NCOMP)
        E["csh_vec_mul_table" + sfx] = (lambda k, fn=fn, st=st: fn("csh_vec_mul_table")(k.f, a, no(k, b), sz(k.n), u32(k.ncomp), *st), CURVE + NCOMP)
        E["csh_rep3_local_mul_vec" + sfx] = (lambda k, fn=fn, st=st: fn("csh_rep3_local_mul_vec")(k.f, a, b, no(k, c), out, sz(k.n), *st), CURVE)
        E["csh_rep3_to_shamir_vec" + sfx] = (lambda k, fn=fn, st=st: fn("csh_rep3_to_shamir_vec")(k.f, a, no(k, one), one, out, sz(k.n), *st), CURVE)
        E["csh_rep3_masks" + sfx] = (lambda k, fn=fn, st=st: fn("csh_rep3_masks")(k.f, no(k, one), C.c_uint64(0), one, C.c_uint64(0), out, sz(k.n), *st),
                                     CURVE)
        E["csh_lincomb" + sfx] = (lambda k, fn=fn, st=st: fn("csh_lincomb")(k.f, _ptrs([B.a, B.b]), no(k, one), sz(2), out, sz(k.n), *st), CURVE)
        E["csh_vec_prefix_prod" + sfx] = (lambda k, fn=fn, st=st: fn("csh_vec_prefix_prod")(k.f, no(k, a), out, sz(k.n), *st), CURVE)
        E["csh_vec_batch_inverse" + sfx] = (lambda k, fn=fn, st=st: fn("csh_vec_batch_inverse")(k.f, a, no(k, out), sz(k.n), None, *st), CURVE)
        E["csh_eval_poly" + sfx] = (lambda k, fn=fn, st=st: fn("csh_eval_poly")(k.f, a, sz(k.n), u32(k.ncomp), no(k, one), out, *st), CURVE + NCOMP)
        E["csh_mle_fold" + sfx] = (lambda k, fn=fn, st=st: fn("csh_mle_fold")(k.f, _ptrs([B.a, B.b], hole(k, 1)), _ptrs([B.a, B.out2] if k.in_place else [B.out, B.out2]),
                                                                             sz(2), sz(k.n), u32(k.ncomp), one, *st), CURVE + NCOMP + ("in_place",))
        E["csh_mle_fold_rounds" + sfx] = (lambda k, fn=fn, st=st: fn("csh_mle_fold_rounds")(k.f, a, sz(k.n), u32(k.ncomp), no(k, one), sz(2), a if k.in_place else out,
                                                                                           None, *st), CURVE + NCOMP + ("in_place",))
        E["csh_bit_reverse" + sfx] = (lambda k, fn=fn, st=st: fn("csh_bit_reverse")(k.f, a, u32(3), u32(k.ncomp), *st), ("grumpkin", "unknown") + NCOMP)
        for op in ("csh_ifft_in_to_out", "csh_fft_out_to_in", "csh_fft", "csh_ifft"):
            E[op + sfx] = (lambda k, fn=fn, st=st, op=op: fn(op)(no(k, B.fake_dom), a, u32(2 if k.null else k.ncomp), *st), ("null",) + NCOMP)
    E["csh_poly_div_linear_dev"] = (lambda k: L.csh_poly_div_linear_dev(k.f, a, sz(k.n), u32(k.ncomp), no(k, one), None, None, int(k.in_place),
                                                                        a if k.in_place else out, None, None), CURVE + NCOMP + ("in_place",))
    E["csh_poly_div_linear"] = (lambda k: L.csh_poly_div_linear(k.f, a, sz(k.n), u32(k.ncomp), no(k, one), None, out, None), CURVE + NCOMP)
    pq = lambda k: (B.fake_dom, u32(1), u32(0))
    E["csh_plonk_quot_blinders_dev"] = (lambda k: L.csh_plonk_quot_blinders_dev(*pq(k), one, _ptrs(B.outs[:5], hole(k, 4)), None), ("null",))
    E["csh_plonk_quot_operands_dev"] = (lambda k: L.csh_plonk_quot_operands_dev(*pq(k), _ptrs(B.vecs[:11], hole(k, 10)), _ptrs(B.vecs[:8]), _ptrs(B.vecs[:2]), sz(2),
                                                                                one, one, _ptrs(B.outs), None), ("null",))
    E["csh_plonk_quot_combine_dev"] = (lambda k: L.csh_plonk_quot_combine_dev(*pq(k), _ptrs(B.vecs), a, one, _ptrs(B.outs[:2], hole(k, 1)), None), ("null",))
    E["csh_plonk_quot_finish_dev"] = (lambda k: L.csh_plonk_quot_finish_dev(k.f, sz(k.n), u32(1), u32(0), a, no(k, b), one, a if k.in_place else out, _p(B.out2),
                                                                            c, None), CURVE + ("in_place",))
    E["csh_matrix_upload"] = (lambda k: L.csh_matrix_upload(k.f, no(k, _p(B.row_ptr)), None, None, sz(1), sz(0), C.byref(B.handle)), ("grumpkin", "unknown", "null"))
    E["csh_domain_create"] = (lambda k: L.csh_domain_create(k.f, u32(3), None, None if k.null else C.byref(B.handle)), ("grumpkin", "unknown", "null"))
    return E


DEVICE = (NO_DEVICE, b"no HIP device")
EXPECTED = {
    "csh_bit_reverse": {"grumpkin": DEVICE, "unknown": DEVICE, "ncomp0": DEVICE, "ncomp3": DEVICE},
    "csh_bit_reverse_dev": {"grumpkin": (INVALID, b'unknown curve'), "unknown": (INVALID, b'unknown curve'),
                           "ncomp0": (INVALID, b'ncomp must be 1 or 2'), "ncomp3": (INVALID, b'ncomp must be 1 or 2')},
    "csh_domain_create": {"grumpkin": DEVICE, "unknown": DEVICE, "null": (INVALID, b'out is NULL')},
    "csh_eval_poly": {"grumpkin": (INVALID, b'field_of: BN254, BLS12-381 or BLS12-377'),
                     "unknown": (INVALID, b'field_of: BN254, BLS12-381 or BLS12-377'), "n_big": (INVALID, b'n exceeds 2^28, the largest domain'),
                     "null": (INVALID, b'eval_poly: NULL argument'), "ncomp0": (INVALID, b'ncomp must be 1 or 2'),
                     "ncomp3": (INVALID, b'ncomp must be 1 or 2')},
    "csh_eval_poly_dev": {"grumpkin": (INVALID, b'field_of: BN254, BLS12-381 or BLS12-377'),
                         "unknown": (INVALID, b'field_of: BN254, BLS12-381 or BLS12-377'), "n_big": (INVALID, b'n exceeds 2^28, the largest domain'),
                         "null": (INVALID, b'eval_poly: NULL argument'), "ncomp0": (INVALID, b'ncomp must be 1 or 2'),
                         "ncomp3": (INVALID, b'ncomp must be 1 or 2')},
    "csh_fft": {"null": (INVALID, b'domain is NULL'), "ncomp0": (INVALID, b'ncomp must be 1 or 2'), "ncomp3": (INVALID, b'ncomp must be 1 or 2')},
    "csh_fft_dev": {"null": (INVALID, b'domain is NULL'), "ncomp0": (INVALID, b'ncomp must be 1 or 2'), "ncomp3": (INVALID, b'ncomp must be 1 or 2')},
    "csh_fft_out_to_in": {"null": (INVALID, b'domain is NULL'), "ncomp0": (INVALID, b'ncomp must be 1 or 2'),
                         "ncomp3": (INVALID, b'ncomp must be 1 or 2')},
    "csh_fft_out_to_in_dev": {"null": (INVALID, b'domain is NULL'), "ncomp0": (INVALID, b'ncomp must be 1 or 2'),
                             "ncomp3": (INVALID, b'ncomp must be 1 or 2')},
    "csh_ifft": {"null": (INVALID, b'domain is NULL'), "ncomp0": (INVALID, b'ncomp must be 1 or 2'), "ncomp3": (INVALID, b'ncomp must be 1 or 2')},
    "csh_ifft_dev": {"null": (INVALID, b'domain is NULL'), "ncomp0": (INVALID, b'ncomp must be 1 or 2'), "ncomp3": (INVALID, b'ncomp must be 1 or 2')},
    "csh_ifft_in_to_out": {"null": (INVALID, b'domain is NULL'), "ncomp0": (INVALID, b'ncomp must be 1 or 2'),
                          "ncomp3": (INVALID, b'ncomp must be 1 or 2')},
    "csh_ifft_in_to_out_dev": {"null": (INVALID, b'domain is NULL'), "ncomp0": (INVALID, b'ncomp must be 1 or 2'),
                              "ncomp3": (INVALID, b'ncomp must be 1 or 2')},
    "csh_lincomb": {"grumpkin": DEVICE, "unknown": DEVICE, "n_big": DEVICE, "null": (INVALID, b'lincomb: NULL argument')},
    "csh_lincomb_dev": {"grumpkin": DEVICE, "unknown": DEVICE, "n_big": DEVICE, "null": (INVALID, b'lincomb: NULL argument')},
    "csh_matrix_upload": {"grumpkin": (INVALID, b'unknown curve'), "unknown": (INVALID, b'unknown curve'),
                         "null": (INVALID, b'matrix_upload: NULL argument')},
    "csh_mle_fold": {"grumpkin": (INVALID, b'field_of: BN254, BLS12-381 or BLS12-377'),
                    "unknown": (INVALID, b'field_of: BN254, BLS12-381 or BLS12-377'), "n_big": (INVALID, b'n exceeds 2^28, the largest domain'),
                    "null": (INVALID, b'mle_fold: NULL argument'), "ncomp0": (INVALID, b'ncomp must be 1 or 2'),
                    "ncomp3": (INVALID, b'ncomp must be 1 or 2'), "in_place": (INVALID, b'mle_fold: an output overlaps')},
    "csh_mle_fold_dev": {"grumpkin": (INVALID, b'field_of: BN254, BLS12-381 or BLS12-377'),
                        "unknown": (INVALID, b'field_of: BN254, BLS12-381 or BLS12-377'), "n_big": (INVALID, b'n exceeds 2^28, the largest domain'),
                        "null": (INVALID, b'mle_fold: NULL argument'), "ncomp0": (INVALID, b'ncomp must be 1 or 2'),
                        "ncomp3": (INVALID, b'ncomp must be 1 or 2'), "in_place": (INVALID, b'mle_fold: an output overlaps')},
    "csh_mle_fold_rounds": {"grumpkin": (INVALID, b'field_of: BN254, BLS12-381 or BLS12-377'),
                           "unknown": (INVALID, b'field_of: BN254, BLS12-381 or BLS12-377'), "n_big": (INVALID, b'n exceeds 2^28, the largest domain'),
                           "null": (INVALID, b'mle_fold_rounds: NULL argument'), "ncomp0": (INVALID, b'ncomp must be 1 or 2'),
                           "ncomp3": (INVALID, b'ncomp must be 1 or 2'), "in_place": (INVALID, b'mle_fold_rounds: an output overlaps')},
    "csh_mle_fold_rounds_dev": {"grumpkin": (INVALID, b'field_of: BN254, BLS12-381 or BLS12-377'),
                               "unknown": (INVALID, b'field_of: BN254, BLS12-381 or BLS12-377'),
                               "n_big": (INVALID, b'n exceeds 2^28, the largest domain'), "null": (INVALID, b'mle_fold_rounds: NULL argument'),
                               "ncomp0": (INVALID, b'ncomp must be 1 or 2'), "ncomp3": (INVALID, b'ncomp must be 1 or 2'),
                               "in_place": (INVALID, b'mle_fold_rounds: an output overlaps')},
    "csh_plonk_quot_blinders_dev": {"null": (INVALID, b'plonk_quot_blinders: NULL argument')},
    "csh_plonk_quot_combine_dev": {"null": (INVALID, b'plonk_quot_combine: NULL argument')},
    "csh_plonk_quot_finish_dev": {"grumpkin": (INVALID, b'plonk_quot_finish: field_of must be BN254, BLS12-381 or BLS12-377'),
                                 "unknown": (INVALID, b'plonk_quot_finish: field_of must be BN254, BLS12-381 or BLS12-377'),
                                 "n_big": (INVALID, b'plonk_quot_finish: n must be a power of two, 8 .. 2^26'),
                                 "null": (INVALID, b'plonk_quot_finish: NULL argument'),
                                 "in_place": (INVALID, b'plonk_quot_finish: an output overlaps an input')},
    "csh_plonk_quot_operands_dev": {"null": (INVALID, b'plonk_quot_operands: NULL argument')},
    "csh_poly_div_linear": {"grumpkin": (INVALID, b'field_of: BN254, BLS12-381 or BLS12-377'),
                           "unknown": (INVALID, b'field_of: BN254, BLS12-381 or BLS12-377'), "n_big": (INVALID, b'n exceeds 2^28, the largest domain'),
                           "null": (INVALID, b'poly_div_linear: NULL argument'), "ncomp0": (INVALID, b'ncomp must be 1 or 2'),
                           "ncomp3": (INVALID, b'ncomp must be 1 or 2')},
    "csh_poly_div_linear_dev": {"grumpkin": (INVALID, b'field_of: BN254, BLS12-381 or BLS12-377'),
                               "unknown": (INVALID, b'field_of: BN254, BLS12-381 or BLS12-377'),
                               "n_big": (INVALID, b'n exceeds 2^28, the largest domain'), "null": (INVALID, b'poly_div_linear: NULL argument'),
                               "ncomp0": (INVALID, b'ncomp must be 1 or 2'), "ncomp3": (INVALID, b'ncomp must be 1 or 2'),
                               "in_place": (INVALID, b'poly_div_linear: accumulate needs out != in')},
    "csh_rep3_local_mul_vec": {"grumpkin": DEVICE, "unknown": DEVICE, "n_big": DEVICE, "null": DEVICE},
    "csh_rep3_local_mul_vec_dev": {"grumpkin": DEVICE, "unknown": DEVICE, "n_big": DEVICE,
                                  "null": (INVALID, b'rep3_local_mul_vec: Rep3 (protocol 1) needs its masks')},
    "csh_rep3_masks": {"grumpkin": DEVICE, "unknown": DEVICE, "n_big": DEVICE, "null": DEVICE},
    "csh_rep3_masks_dev": {"grumpkin": DEVICE, "unknown": DEVICE, "n_big": DEVICE, "null": (INVALID, b'rep3_masks: NULL argument')},
    "csh_rep3_to_shamir_vec": {"grumpkin": DEVICE, "unknown": DEVICE, "n_big": DEVICE, "null": DEVICE},
    "csh_rep3_to_shamir_vec_dev": {"grumpkin": DEVICE, "unknown": DEVICE, "n_big": DEVICE, "null": (INVALID, b'translation points are NULL')},
    "csh_vec_add": {"grumpkin": DEVICE, "unknown": DEVICE, "n_big": DEVICE, "null": DEVICE, "ncomp0": DEVICE, "ncomp3": DEVICE},
    "csh_vec_add_dev": {"grumpkin": DEVICE, "unknown": DEVICE, "n_big": DEVICE, "null": DEVICE, "ncomp0": DEVICE, "ncomp3": DEVICE},
    "csh_vec_batch_inverse": {"grumpkin": (INVALID, b'field_of: BN254, BLS12-381 or BLS12-377'),
                             "unknown": (INVALID, b'field_of: BN254, BLS12-381 or BLS12-377'),
                             "n_big": (INVALID, b'n exceeds 2^28, the largest domain'), "null": (INVALID, b'vec_batch_inverse: NULL argument')},
    "csh_vec_batch_inverse_dev": {"grumpkin": (INVALID, b'field_of: BN254, BLS12-381 or BLS12-377'),
                                 "unknown": (INVALID, b'field_of: BN254, BLS12-381 or BLS12-377'),
                                 "n_big": (INVALID, b'n exceeds 2^28, the largest domain'), "null": (INVALID, b'vec_batch_inverse: NULL argument')},
    "csh_vec_mul": {"grumpkin": DEVICE, "unknown": DEVICE, "n_big": DEVICE, "null": DEVICE},
    "csh_vec_mul_dev": {"grumpkin": DEVICE, "unknown": DEVICE, "n_big": DEVICE, "null": DEVICE},
    "csh_vec_mul_table": {"grumpkin": DEVICE, "unknown": DEVICE, "n_big": DEVICE, "null": DEVICE, "ncomp0": DEVICE, "ncomp3": DEVICE},
    "csh_vec_mul_table_dev": {"grumpkin": DEVICE, "unknown": DEVICE, "n_big": DEVICE, "null": DEVICE, "ncomp0": (INVALID, b'ncomp must be 1 or 2'),
                             "ncomp3": (INVALID, b'ncomp must be 1 or 2')},
    "csh_vec_prefix_prod": {"grumpkin": (INVALID, b'field_of: BN254, BLS12-381 or BLS12-377'),
                           "unknown": (INVALID, b'field_of: BN254, BLS12-381 or BLS12-377'), "n_big": (INVALID, b'n exceeds 2^28, the largest domain'),
                           "null": (INVALID, b'vec_prefix_prod: NULL argument')},
    "csh_vec_prefix_prod_dev": {"grumpkin": (INVALID, b'field_of: BN254, BLS12-381 or BLS12-377'),
                               "unknown": (INVALID, b'field_of: BN254, BLS12-381 or BLS12-377'),
                               "n_big": (INVALID, b'n exceeds 2^28, the largest domain'), "null": (INVALID, b'vec_prefix_prod: NULL argument')},
    "csh_vec_sub": {"grumpkin": DEVICE, "unknown": DEVICE, "n_big": DEVICE, "null": DEVICE, "ncomp0": DEVICE, "ncomp3": DEVICE},
    "csh_vec_sub_dev": {"grumpkin": DEVICE, "unknown": DEVICE, "n_big": DEVICE, "null": DEVICE, "ncomp0": DEVICE, "ncomp3": DEVICE},
}


def _rows():
    return [(name, case) for name, cases in sorted(EXPECTED.items()) for case in cases]


def test_the_table_has_a_row_for_every_case_of_every_entry_point(hip):
    E = _entry_points(hip.lib(), Bufs())
    assert sorted(E) == sorted(EXPECTED)
    for name, (_, cases) in E.items():
        assert sorted(cases) == sorted(EXPECTED[name]), name


def _check(hip, want_device):
    L, B = hip.lib(), Bufs()
    E = _entry_points(L, B)
    seen = 0
    for name, case in _rows():
        status, text = EXPECTED[name][case]
        if (status == NO_DEVICE) != want_device:
            continue
        rc = E[name][0](Case(case))
        assert rc == status and text in L.csh_last_error(), (name, case, rc, L.csh_last_error())
        seen += 1
    assert seen


def test_refusals_that_come_before_the_device(hip):
    """The rows that read CSH_ERR_INVALID: refused on the host, on any machine, with the text that names the rule."""
    _check(hip, False)


def test_arguments_that_are_looked_at_after_the_device(hip):
    """The rows that read CSH_ERR_NO_DEVICE: the entry point asks for the device first. (With a device these calls would go on to read host
    memory from a kernel; what they answer there for a curve they do not know is in tests/test_gpu_fr_layer.py.)"""
    if hip.have_device():
        pytest.skip("a HIP device is present")
    _check(hip, True)
