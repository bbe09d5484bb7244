"""With a device present and valid 8-element device buffers, every *_dev entry point of vec_ops, field_scan, mle_fold, plonk_quot and ntt
that takes a curve (and the two calls of sparse and ntt that make a handle for one) refuses Grumpkin and a value that is no curve with
CSH_ERR_INVALID, on the host: nothing is launched, and the output buffer holds afterwards what it held before. The refusals that need no
device are tests/test_fr_layer_cpu.py."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
INVALID = -1
GRUMPKIN, NO_CURVE = 2, 99
PATTERN = 0xA5A5A5A5A5A5A5A5


def test_every_dev_entry_point_refuses_a_curve_without_scalar_field_entry_points(gpu):
    L = gpu.lib()
    n, words = 8, 4 * 2 * 8   # 8 elements of two components
    sz, u32, u64 = C.c_size_t, C.c_uint32, C.c_uint64
    ones = np.tile(np.array([1, 0, 0, 0], dtype=np.uint64), 2 * n)
    d_a, d_b, d_c = (gpu.DeviceBuffer.from_host(ones) for _ in range(3))
    d_out, d_out2 = (gpu.DeviceBuffer.from_host(np.full(words, PATTERN, dtype=np.uint64)) for _ in range(2))
    a, b, c, out, out2 = (d.ptr for d in (d_a, d_b, d_c, d_out, d_out2))
    host = np.ones(4 * 8, dtype=np.uint64)   # a point, a root, challenges, seeds, coefficients
    hp = host.ctypes.data_as(C.c_void_p)
    ptrs = lambda *ps: (C.c_void_p * len(ps))(*[p.value for p in ps])
    handle = C.c_void_p(0)
    row_ptr = np.zeros(2, dtype=np.uint64)
    calls = {
        "csh_vec_mul_dev": lambda f: L.csh_vec_mul_dev(f, a, b, out, sz(n), None),
        "csh_vec_add_dev": lambda f: L.csh_vec_add_dev(f, a, b, out, sz(n), u32(2), None),
        "csh_vec_sub_dev": lambda f: L.csh_vec_sub_dev(f, a, b, out, sz(n), u32(2), None),
        "csh_vec_mul_table_dev": lambda f: L.csh_vec_mul_table_dev(f, out, a, sz(n), u32(2), None),
        "csh_rep3_local_mul_vec_dev": lambda f: L.csh_rep3_local_mul_vec_dev(f, a, b, c, out, sz(n), None),
        "csh_rep3_to_shamir_vec_dev": lambda f: L.csh_rep3_to_shamir_vec_dev(f, a, hp, hp, out, sz(n), None),
        "csh_rep3_masks_dev": lambda f: L.csh_rep3_masks_dev(f, hp, u64(0), hp, u64(0), out, sz(n), None),
        "csh_lincomb_dev": lambda f: L.csh_lincomb_dev(f, ptrs(a, b), hp, sz(2), out, sz(n), None),
        "csh_vec_prefix_prod_dev": lambda f: L.csh_vec_prefix_prod_dev(f, a, out, sz(n), None),
        "csh_vec_batch_inverse_dev": lambda f: L.csh_vec_batch_inverse_dev(f, a, out, sz(n), None, None),
        "csh_eval_poly_dev": lambda f: L.csh_eval_poly_dev(f, a, sz(n), u32(2), hp, out, None),
        "csh_poly_div_linear_dev": lambda f: L.csh_poly_div_linear_dev(f, a, sz(n), u32(2), hp, None, None, 0, out, out2, None),
        "csh_mle_fold_dev": lambda f: L.csh_mle_fold_dev(f, ptrs(a, b), ptrs(out, out2), sz(2), sz(n), u32(2), hp, None),
        "csh_mle_fold_rounds_dev": lambda f: L.csh_mle_fold_rounds_dev(f, a, sz(n), u32(2), hp, sz(2), out, out2, None),
        "csh_plonk_quot_finish_dev": lambda f: L.csh_plonk_quot_finish_dev(f, sz(8), u32(0), u32(0), a, b, hp, out, out2, c, None),
        "csh_bit_reverse_dev": lambda f: L.csh_bit_reverse_dev(f, out, u32(3), u32(2), None),
        "csh_matrix_upload": lambda f: L.csh_matrix_upload(f, row_ptr.ctypes.data_as(C.c_void_p), None, None, sz(1), sz(0), C.byref(handle)),
        "csh_domain_create": lambda f: L.csh_domain_create(f, u32(3), None, C.byref(handle)),
    }
    for name, call in calls.items():
        for f in (GRUMPKIN, NO_CURVE):
            rc = call(f)
            assert rc == INVALID, (name, f, rc, L.csh_last_error())
            assert b"curve" in L.csh_last_error() or b"field_of" in L.csh_last_error(), (name, f, L.csh_last_error())
            assert not handle.value, name
    for d in (d_out, d_out2):
        assert np.all(d.to_host() == PATTERN)
    for d in (d_a, d_b, d_c):
        assert np.array_equal(d.to_host(), ones)
