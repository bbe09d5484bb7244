"""CPU tests of the multilinear folds (csrc/mle_fold.hip: csh_mle_fold, csh_mle_fold_rounds): the C boundary without a device, and the
arithmetic itself -- the launches, tiles and lazy rounds of k_mle_fold_rounds and the sweeps of k_mle_fold -- run on the host from the same
templates the gfx950 kernels instantiate, with the limb-bound contract checks of selftest.hip on (a violated bound aborts the process, so
"the checks are silent" is the test finishing at all). Truth is the reference's loops restated in Python integers."""
import ctypes as C
import re

import numpy as np
import pytest

from tests import helpers as H

CURVES = ["bn254", "bls12_381", "bls12_377"]
FOLD_CITES = ["co-noir/co-ultrahonk/src/co_decider/co_sumcheck/co_sumcheck_prover.rs:34-98", "co-noir/ultrahonk/src/decider/sumcheck/sumcheck_prover.rs:20-60",
              "partially_evaluate_init", "partially_evaluate_inplace"]
ROUNDS_CITES = ["co_shplemini_prover.rs:236-312", "shplemini_prover.rs:198", "co-noir-common/src/polynomials/polynomial.rs:270-312",
                "shared_polynomial.rs:154-199", "co_sumcheck_prover.rs:435", "sumcheck_prover.rs:334", "compute_fold_polynomials", "evaluate_mle"]
PAIRS = [("csh_mle_fold_dev", "csh_mle_fold", FOLD_CITES), ("csh_mle_fold_rounds_dev", "csh_mle_fold_rounds", ROUNDS_CITES)]
NO_DEVICE, INVALID = -2, -1


def reference_fold(p, poly, round_challenge):
    """The reference's loop as the reference writes it (co_sumcheck_prover.rs:48-50, co_shplemini_prover.rs:260-269)."""
    out = [0] * (len(poly) // 2)
    for i in range(0, len(poly), 2):
        out[i >> 1] = (poly[i] + (poly[i + 1] - poly[i]) * round_challenge) % p
    return out


def reference_levels(p, poly, challenges):
    """compute_fold_polynomials' chain (co_shplemini_prover.rs:251-274), every level kept."""
    levels, a_l = [], poly
    for u_l in challenges:
        a_l = reference_fold(p, a_l, u_l)
        levels.append(a_l)
    return levels


def reference_evaluate_mle(p, coefficients, evaluation_points):
    """Polynomial::evaluate_mle (polynomial.rs:270-312) for len(coefficients) = 2^dim, dim <= len(evaluation_points)."""
    dim = (len(coefficients) - 1).bit_length()
    tmp = list(coefficients)
    for val in evaluation_points[:dim]:
        tmp = reference_fold(p, tmp, val)
    result = tmp[0]
    for point in evaluation_points[dim:]:
        result = result * (1 - point) % p
    return result


def test_header_declares_the_entry_points_with_their_reference_lines(hip):
    """The four prototypes are in include/cosnarks_hip.h and exported, and the comment above each pair cites the reference lines."""
    from cosnarks_amd import bindings
    txt = open(bindings.header_path()).read()
    declared = bindings.declared_symbols()
    L = hip.lib()
    for dev, host, cites in PAIRS:
        for name in (dev, host):
            assert name in declared and hasattr(L, name), name
        at = txt.index("int %s(" % dev)
        comment = txt[txt.rindex("/*", 0, at):at]
        for c in cites:
            assert c in comment, (dev, c)
        assert at < txt.index("int %s(" % host)
    assert not hasattr(bindings, "selftest_mle_fold_host") and "csh_selftest_mle_fold_host" not in declared
    assert hasattr(L, "csh_selftest_mle_fold_host")


def _p(x):
    return x.ctypes.data_as(C.c_void_p) if x is not None else None


def _ptrs(*arrs):
    return (C.c_void_p * len(arrs))(*[a.ctypes.data if a is not None else None for a in arrs])


def _bufs():
    a = np.zeros(16 * 2 * 4, dtype=np.uint64)
    out = np.zeros(16 * 2 * 4, dtype=np.uint64)
    u = np.ones(4 * 4, dtype=np.uint64)
    return a, out, u


def test_argument_checks_come_before_the_device(hip):
    """Every argument rule answers CSH_ERR_INVALID with a message that names it, in both forms, on any machine."""
    L = hip.lib()
    a, out, u = _bufs()
    b = np.zeros_like(a)
    err = lambda: L.csh_last_error()
    sz = C.c_size_t

    def fold(f, ins, outs, k, n, ncomp, uu, msg):
        for rc in (L.csh_mle_fold_dev(f, ins, outs, sz(k), sz(n), ncomp, uu, None), L.csh_mle_fold(f, ins, outs, sz(k), sz(n), ncomp, uu)):
            assert rc == INVALID and msg in err(), (rc, msg, err())

    def rounds(f, i, n, ncomp, uu, m, lv, la, msg):
        for rc in (L.csh_mle_fold_rounds_dev(f, i, sz(n), ncomp, uu, sz(m), lv, la, None), L.csh_mle_fold_rounds(f, i, sz(n), ncomp, uu, sz(m), lv, la)):
            assert rc == INVALID and msg in err(), (rc, msg, err())

    for bad_curve in (2, 7):  # Grumpkin has no scalar-field entry points; 7 is no curve
        fold(bad_curve, _ptrs(a), _ptrs(out), 1, 8, 1, _p(u), b"field_of")
        rounds(bad_curve, _p(a), 8, 1, _p(u), 2, _p(out), None, b"field_of")
    for f in (0, 1, 3):
        for ncomp in (0, 3):
            fold(f, _ptrs(a), _ptrs(out), 1, 8, ncomp, _p(u), b"ncomp")
            rounds(f, _p(a), 8, ncomp, _p(u), 2, _p(out), None, b"ncomp")
        fold(f, _ptrs(a), _ptrs(out), 1, (1 << 28) + 2, 1, _p(u), b"2^28")
        rounds(f, _p(a), 1 << 29, 1, _p(u), 2, _p(out), None, b"2^28")
        for n in (0, 1, 7):
            fold(f, _ptrs(a), _ptrs(out), 1, n, 1, _p(u), b"even")
        fold(f, _ptrs(a), _ptrs(out), 0, 8, 1, _p(u), b"k must be at least 1")
        fold(f, None, _ptrs(out), 1, 8, 1, _p(u), b"NULL")
        fold(f, _ptrs(a), None, 1, 8, 1, _p(u), b"NULL")
        fold(f, _ptrs(a), _ptrs(out), 1, 8, 1, None, b"NULL")
        fold(f, _ptrs(a, None), _ptrs(out, b), 2, 8, 1, _p(u), b"NULL")
        fold(f, _ptrs(a, b), _ptrs(out, None), 2, 8, 1, _p(u), b"NULL")
        for m, n in ((0, 8), (4, 8), (2, 6), (3, 12), (1, 0), (29, 1 << 28)):
            rounds(f, _p(a), n, 1, _p(u), m, _p(out), None, b"2^m must divide n")
        rounds(f, None, 8, 1, _p(u), 2, _p(out), None, b"NULL")
        rounds(f, _p(a), 8, 1, None, 2, _p(out), None, b"NULL")
        rounds(f, _p(a), 8, 1, _p(u), 2, None, None, b"one of levels and last")
        # overlap: in place, an output inside an input, an output ending where another vector's input has begun
        fold(f, _ptrs(a), _ptrs(a), 1, 8, 2, _p(u), b"overlaps")
        fold(f, _ptrs(a), _ptrs(a[4 * 15:]), 1, 8, 2, _p(u), b"overlaps")
        fold(f, _ptrs(a, b), _ptrs(out, a[4:]), 2, 8, 1, _p(u), b"overlaps")
        rounds(f, _p(a), 8, 1, _p(u), 2, _p(a), None, b"overlaps")
        rounds(f, _p(a), 8, 1, _p(u), 2, _p(out), _p(a[4 * 7:]), b"overlaps")
        rounds(f, _p(a[4 * 5:]), 8, 1, _p(u), 2, _p(a), None, b"overlaps")  # levels: 6 elements from a[0], the input starts at element 5
    for bad in (2, 0, 12, -3):
        assert hip.lib().csh_tune_set(b"fold_tile_log", bad) == INVALID and b"fold_tile_log" in err()
    assert hip.tune_get("fold_tile_log") == 10
    for good in (3, 11, 10):
        hip.tune_set("fold_tile_log", good)
        assert hip.tune_get("fold_tile_log") == good


def test_no_device_no_result(hip):
    """Without a device every valid call fails with the no-device error: there is no CPU path."""
    if hip.have_device():
        pytest.skip("a HIP device is present")
    L = hip.lib()
    a, out, u = _bufs()
    b, out2 = np.zeros_like(a), np.zeros_like(a)
    sz = C.c_size_t
    for f in (0, 1, 3):
        for rc in (L.csh_mle_fold_dev(f, _ptrs(a, b, a), _ptrs(out, out2, out2[64:]), sz(3), sz(8), 2, _p(u), None),
                   L.csh_mle_fold(f, _ptrs(a), _ptrs(out), sz(1), sz(2), 1, _p(u)),
                   L.csh_mle_fold_dev(f, _ptrs(a[16:]), _ptrs(a), sz(1), sz(8), 1, _p(u), None),   # adjacent, not overlapping
                   L.csh_mle_fold_rounds_dev(f, _p(a), sz(16), 2, _p(u), sz(4), _p(out), None, None),
                   L.csh_mle_fold_rounds_dev(f, _p(a), sz(12), 1, _p(u), sz(2), None, _p(out), None),
                   L.csh_mle_fold_rounds(f, _p(a), sz(16), 1, _p(u), sz(3), _p(out), _p(out2)),
                   L.csh_mle_fold_rounds(f, _p(a[4 * 6:]), sz(8), 1, _p(u), sz(2), _p(a), None)):   # levels end where the input begins
            assert rc == NO_DEVICE
            assert re.search(b"no HIP device|no CPU fallback", L.csh_last_error())
    with pytest.raises(hip.CoSnarksHipError, match="no HIP device|no CPU fallback"):
        hip.mle_fold(hip.BN254, [a], u[:4])
    with pytest.raises(hip.CoSnarksHipError, match="no HIP device|no CPU fallback"):
        hip.mle_fold_rounds(hip.BN254, a, u[:8])


def _fold_host(hip, curve, vals, ncomp, tile_log, us):
    """vals: n x ncomp integers, interleaved -> the levels 1..m (interleaved alike) from csh_selftest_mle_fold_host."""
    F = H.FR[curve]
    n, m = len(vals) // ncomp, len(us)
    a, u = H.pack(F, vals), H.pack(F, us)
    out = np.zeros(4 * ncomp * (n - (n >> m)), dtype=np.uint64)
    rc = hip.lib().csh_selftest_mle_fold_host(H.CURVE_IDS[curve], _p(a), C.c_size_t(n), C.c_uint32(ncomp), tile_log, _p(u), C.c_size_t(m), _p(out))
    assert rc == 0, rc
    H.assert_canonical(F, out)
    flat = H.unpack(F, out)
    return [flat[ncomp * (n - (n >> (l - 1))):ncomp * (n - (n >> l))] for l in range(1, m + 1)]


def _want(F, vals, ncomp, us):
    per_comp = [reference_levels(F.p, vals[c::ncomp], us) for c in range(ncomp)]
    want = []
    for l in range(len(us)):
        lv = [None] * (ncomp * len(per_comp[0][l]))
        for c in range(ncomp):
            lv[c::ncomp] = per_comp[c][l]
        want.append(lv)
    return want


SIZES = [2, 4, 6, 8, 12, 16, 24, 32, 40, 48, 64, 80, 96, 128, 160, 192]   # up to 3 * 2^6, every m with 2^m | n


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("ncomp", [1, 2])
@pytest.mark.parametrize("tile_log", [3, 4, 10])
def test_tiles_and_rounds_known_answers(hip, curve, ncomp, tile_log):
    """The kernels' arithmetic tile after tile on the host, bound checks on: edge values followed by random ones, challenges 0, 1, p - 1 and
    random in every position, every n of SIZES with every m from 1 to the largest with 2^m | n."""
    F = H.FR[curve]
    r = H.rng(700 + tile_log)
    edge = [v % F.p for v in H.edge_elems(F)]
    pool = [0, 1, F.p - 1] + H.rand_elems(F, 5, r)
    case = 0
    for n in SIZES:
        vals = (edge * ncomp + H.rand_elems(F, n * ncomp, r))[:n * ncomp]
        for m in range(1, 9):
            if n % (1 << m):
                break
            us = [pool[(case + 3 * i) % len(pool)] for i in range(m)]
            case += 1
            assert _fold_host(hip, curve, vals, ncomp, tile_log, us) == _want(F, vals, ncomp, us), (curve, ncomp, tile_log, n, m)
    L = hip.lib()
    assert L.csh_selftest_mle_fold_host(H.CURVE_IDS[curve], None, C.c_size_t(8), 1, tile_log, None, C.c_size_t(1), None) == INVALID
    a = H.pack(F, [1] * 8)
    assert L.csh_selftest_mle_fold_host(H.CURVE_IDS[curve], _p(a), C.c_size_t(6), 1, tile_log, _p(a), C.c_size_t(2), _p(a)) == INVALID
    assert L.csh_selftest_mle_fold_host(H.CURVE_IDS[curve], _p(a), C.c_size_t(8), 1, 12, _p(a), C.c_size_t(2), _p(a)) == INVALID


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("ncomp", [1, 2])
def test_exact_outputs_and_special_challenges(hip, curve, ncomp):
    """u = 0 returns the even entries and u = 1 the odd ones; pairs with b = a fold to a under any challenge; pairs solved for outputs of
    exactly 0, 1 and p - 1 give those words."""
    F = H.FR[curve]
    p = F.p
    r = H.rng(811)
    edge = [v % p for v in H.edge_elems(F)]
    n = 64
    vals = (edge * ncomp * 3 + H.rand_elems(F, n * ncomp, r))[:n * ncomp]
    for tile_log in (3, 10):
        (even,) = _fold_host(hip, curve, vals, ncomp, tile_log, [0])
        (odd,) = _fold_host(hip, curve, vals, ncomp, tile_log, [1])
        for c in range(ncomp):
            assert even[c::ncomp] == vals[c::ncomp][0::2] and odd[c::ncomp] == vals[c::ncomp][1::2]
        for u in (p - 1, 2, r.randrange(p)):
            # b = a
            same = []
            for j in range(n // 2):
                same += [vals[j * ncomp + c] for c in range(ncomp)] * 2
            (got,) = _fold_host(hip, curve, same, ncomp, tile_log, [u])
            assert got == vals[:n // 2 * ncomp]
            # outputs exactly 0, 1, p - 1: b = a + (t - a) / u
            targets = [(0, 1, p - 1)[(j + c) % 3] for j in range(n // 2) for c in range(ncomp)]
            solved = []
            for j in range(n // 2):
                a = [vals[j * ncomp + c] for c in range(ncomp)]
                b = [(a[c] + (targets[j * ncomp + c] - a[c]) * pow(u, -1, p)) % p for c in range(ncomp)]
                solved += a + b
            (got,) = _fold_host(hip, curve, solved, ncomp, tile_log, [u])
            assert got == targets


@pytest.mark.parametrize("curve", CURVES)
def test_longest_on_chip_chain_at_the_top_of_the_field(hip, curve):
    """u = p - 1 on a vector of p - 1, and on p - 1 alternating with 0 (the largest |b - a|), through the longest chain that stays on
    chip (11 rounds at fold_tile_log 11) and the same 11 rounds as four launches of tile 3. Between launches a level is canonical, so no
    value is lazy for more rounds than this through the tiles; test_lazy_bound_is_stable_over_28_rounds goes further on single pairs."""
    F = H.FR[curve]
    p = F.p
    n, m = 1 << 11, 11
    for vals in ([p - 1] * n, [p - 1, 0] * (n // 2), [0, p - 1] * (n // 2)):
        for u in (p - 1, (p - 1) // 2):
            want = _want(F, vals, 1, [u] * m)
            for tile_log in (11, 3):
                assert _fold_host(hip, curve, vals, 1, tile_log, [u] * m) == want, (curve, tile_log, hex(u))
    vals = [p - 1, 0, 0, p - 1] * (n // 4)
    assert _fold_host(hip, curve, vals, 2, 11, [p - 1] * 10) == _want(F, vals, 2, [p - 1] * 10)


@pytest.mark.parametrize("curve", CURVES)
def test_lazy_bound_is_stable_over_28_rounds(hip, curve):
    """fold_step 28 times on lazy values with nothing canonical in between, limb-bound checks on: (x, y) <- (x + u (y - x), y + u (x - y)).
    The worst growth for the lazy bounds is u = p - 1 on p - 1 / p - 1, p - 1 / 0 and 0 / p - 1; other challenges and values ride along.
    Every round's two values equal the Python integers and are canonical."""
    F = H.FR[curve]
    p = F.p
    r = H.rng(913)
    rounds = 28
    pairs = [(p - 1, p - 1), (p - 1, 0), (0, p - 1), (1, p - 2), (r.randrange(p), r.randrange(p))]
    for u in (p - 1, p - 2, (p - 1) // 2, 2, r.randrange(p)):
        for a, b in pairs:
            out = np.zeros(8 * rounds, dtype=np.uint64)
            rc = hip.lib().csh_selftest_fold_step_chain_host(H.CURVE_IDS[curve], _p(H.pack(F, [a])), _p(H.pack(F, [b])), _p(H.pack(F, [u])),
                                                             C.c_size_t(rounds), _p(out))
            assert rc == 0
            want, x, y = [], a, b
            for _ in range(rounds):
                x, y = (x + u * (y - x)) % p, (y + u * (x - y)) % p
                want += [x, y]
            assert H.unpack(F, out) == want, (curve, hex(u), hex(a), hex(b))
    assert hip.lib().csh_selftest_fold_step_chain_host(H.CURVE_IDS[curve], None, None, None, C.c_size_t(1), None) == INVALID
