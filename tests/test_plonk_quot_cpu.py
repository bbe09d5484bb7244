"""CPU tests of the PLONK quotient stages (csrc/plonk_quot.hip: csh_plonk_quot_{blinders,operands,combine,finish}_dev): the C boundary
without a device, and the arithmetic itself run on the host through csh_selftest_plonk_quot_host -- the argument builders and the
per-index functions the gfx950 kernels call, with the limb-bound contract checks of selftest.hip on (a violated bound aborts the process).
Truth is tests/plonk_quot_ref.py, the reference's loops in Python integers. Every comparison is exact."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import helpers as H
from tests import plonk_quot_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = ["bn254", "bls12_381"]
PARTIES = [(0, 0), (1, 0), (1, 1), (1, 2)]   # (protocol, party)
NO_DEVICE, INVALID = -2, -1
ENTRY = {"csh_plonk_quot_blinders_dev": ["round3.rs:269-274", "339-353"], "csh_plonk_quot_operands_dev": ["round3.rs:320-419"],
         "csh_plonk_quot_combine_dev": ["round3.rs:88-105", "435-467"], "csh_plonk_quot_finish_dev": ["round3.rs:468-498"]}
sz, u32 = C.c_size_t, C.c_uint32


def ext_generator(F, n):
    """a generator of the 4 n-point domain"""
    from oracle import ntt
    return ntt.roots_of_unity(F)[1][(4 * n).bit_length() - 1]


def _p(x):
    return x.ctypes.data_as(C.c_void_p) if x is not None else None


def _ptrs(arrs):
    return (C.c_void_p * len(arrs))(*[a.ctypes.data if a is not None else None for a in arrs]) if len(arrs) else None


def _vec(F, v):
    return H.pack(F, R.flat(v))


def _run_host(hip, curve, stage, case, w_ext, ins, scalars, out_lens):
    """csh_selftest_plonk_quot_host for one stage -> the outputs as lists of shares"""
    F, T = H.FR[curve], case["T"]
    outs = [np.full(4 * T.ncomp * k, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64) for k in out_lens]
    sc = H.pack(F, scalars)
    rc = hip.lib().csh_selftest_plonk_quot_host(H.CURVE_IDS[curve], stage, _p(H.pack(F, [w_ext])), sz(case["N"]), u32(T.protocol), u32(T.party),
                                                _ptrs(ins), sz(len(case["buffer_a"])), _p(sc), _ptrs(outs))
    assert rc == 0, rc
    got = []
    for o in outs:
        v = H.unpack(F, o)   # strict: canonical
        got.append([tuple(v[i * T.ncomp:(i + 1) * T.ncomp]) for i in range(len(v) // T.ncomp)])
    return got


def run_all_stages(hip, curve, case, w_ext):
    """The four stages on the host against the restatement's outputs of `case`."""
    F, N, n = H.FR[curve], case["N"], case["n"]
    got = _run_host(hip, curve, 0, case, w_ext, [], R.flat(case["b"][:9]), [N] * 5)
    for name, g, w in zip(["ap", "bp", "cp", "zp", "zwp"], got, case["want_blinders"]):
        assert g == w, ("blinders", name)
    ins = [_vec(F, case["shares"][k]) for k in R.SHARE_NAMES] + [H.pack(F, case["zkey"][k]) for k in R.PUBLIC_NAMES]
    ins += [H.pack(F, l) for l in case["zkey"]["lagrange"]]
    got = _run_host(hip, curve, 1, case, w_ext, ins, R.flat(case["buffer_a"]) + [case["beta"], case["gamma"], case["k1"], case["k2"]], [N] * 10)
    for name, g, w in zip(R.OPERAND_OUTS, got, case["want_operands"]):
        assert g == w, ("operands", name)
    ins = [_vec(F, case["combine"][k]) for k in R.COMBINE_NAMES] + [H.pack(F, case["lagrange1"])]
    got = _run_host(hip, curve, 2, case, w_ext, ins, [case["alpha"]], [N] * 2)
    for name, g, w in zip(["t", "tz"], got, case["want_combine"]):
        assert g == w, ("combine", name)
    got = _run_host(hip, curve, 3, case, w_ext, [_vec(F, case["ct"]), _vec(F, case["ctz"])], R.flat(case["b"][9:11]), [n + 1, n + 1, n + 6])
    for name, g, w in zip(["t1", "t2", "t3"], got, case["want_finish"]):
        assert g == w, ("finish", name)


def test_header_bindings_and_sys_crate_declare_the_entry_points(hip):
    from cosnarks_amd import bindings
    txt = open(bindings.header_path()).read()
    declared = bindings.declared_symbols()
    sys_rs = open(os.path.join(ROOT, "rust", "cosnarks-hip-sys", "src", "lib.rs")).read()
    L = hip.lib()
    for name, cites in ENTRY.items():
        assert name in declared and hasattr(L, name), name
        at = txt.index("int %s(" % name)
        comment = txt[txt.rindex("/*", 0, at):at]
        for c in cites:
            assert c in comment, (name, c)
        assert "pub fn %s(" % name in sys_rs
        assert hasattr(hip, name[4:-4]) and name in open(bindings.__file__).read()
    section = txt[txt.index("circom PLONK quotient"):txt.index("int csh_plonk_quot_blinders_dev(")]
    for c in ["co-circom/co-plonk/src/round3.rs:246-502", "round3.rs:212-242", "arithmetic.rs:41-49", "shamir/arithmetic.rs:45"]:
        assert c in section, c
    assert "csh_selftest_plonk_quot_host" not in declared and hasattr(L, "csh_selftest_plonk_quot_host")
    assert "struct" not in txt[txt.index("circom PLONK quotient"):txt.index("Rep3 correlated masks generated on the device")]


def _abi_bufs(ncomp=2, N=32):
    mk = lambda k, c: [np.zeros(4 * c * N, dtype=np.uint64) for _ in range(k)]
    return {"sh11": mk(11, ncomp), "pub8": mk(8, 1), "lag": mk(2, 1), "out10": mk(10, ncomp), "sh14": mk(14, ncomp), "out5": mk(5, ncomp),
            "out2": mk(2, ncomp), "host": np.ones(4 * 2 * 16, dtype=np.uint64)}


def test_refusals_come_before_the_device(hip):
    """Every rule that can be checked without looking into a domain answers CSH_ERR_INVALID on any machine. (A domain handle only exists
    where a device does: the size of the domain and the overlap rules of the three calls that take one are in tests/test_gpu_plonk_quot.py.)"""
    L = hip.lib()
    b = _abi_bufs()
    fake_dom = C.c_void_p(b["host"].ctypes.data)   # never looked into: each call below is refused before that
    hp = _p(b["host"])
    err = lambda: L.csh_last_error()

    def blinders(dom, pr, pa, bl, outs):
        return L.csh_plonk_quot_blinders_dev(dom, u32(pr), u32(pa), bl, outs, None)

    def operands(dom, pr, pa, sh, pub, lag, npub, ba, ch, outs):
        return L.csh_plonk_quot_operands_dev(dom, u32(pr), u32(pa), sh, pub, lag, sz(npub), ba, ch, outs, None)

    def combine(dom, pr, pa, sh, l1, al, outs):
        return L.csh_plonk_quot_combine_dev(dom, u32(pr), u32(pa), sh, l1, al, outs, None)

    def finish(f, n, pr, pa, ct, ctz, bb, t1, t2, t3):
        return L.csh_plonk_quot_finish_dev(f, sz(n), u32(pr), u32(pa), ct, ctz, bb, t1, t2, t3, None)

    sh11, pub8, lag, out10, sh14, out5, out2 = (_ptrs(b[k]) for k in ("sh11", "pub8", "lag", "out10", "sh14", "out5", "out2"))
    l1 = _p(b["lag"][0])
    n = 8
    ct, ctz = np.zeros(4 * 2 * 4 * n, dtype=np.uint64), np.zeros(4 * 2 * 4 * n, dtype=np.uint64)
    t1, t2, t3 = (np.zeros(4 * 2 * (n + k), dtype=np.uint64) for k in (1, 1, 6))
    # protocol and party
    for pr, pa in ((2, 0), (0, 3), (1, 3), (7, 7)):
        for rc in (blinders(fake_dom, pr, pa, hp, out5), operands(fake_dom, pr, pa, sh11, pub8, lag, 2, hp, hp, out10),
                   combine(fake_dom, pr, pa, sh14, l1, hp, out2), finish(0, n, pr, pa, _p(ct), _p(ctz), hp, _p(t1), _p(t2), _p(t3))):
            assert rc == INVALID and b"protocol" in err(), (rc, err())
    # NULL pointers, the arrays and their entries
    hole = lambda arrs, k: _ptrs(arrs[:k] + [None] + arrs[k + 1:])
    calls = [blinders(None, 1, 0, hp, out5), blinders(fake_dom, 1, 0, None, out5), blinders(fake_dom, 1, 0, hp, None),
             blinders(fake_dom, 1, 0, hp, hole(b["out5"], 4)),
             operands(None, 1, 0, sh11, pub8, lag, 2, hp, hp, out10), operands(fake_dom, 1, 0, None, pub8, lag, 2, hp, hp, out10),
             operands(fake_dom, 1, 0, sh11, None, lag, 2, hp, hp, out10), operands(fake_dom, 1, 0, sh11, pub8, None, 2, hp, hp, out10),
             operands(fake_dom, 1, 0, sh11, pub8, lag, 2, None, hp, out10), operands(fake_dom, 1, 0, sh11, pub8, lag, 2, hp, None, out10),
             operands(fake_dom, 1, 0, sh11, pub8, lag, 2, hp, hp, None), operands(fake_dom, 1, 0, hole(b["sh11"], 10), pub8, lag, 2, hp, hp, out10),
             operands(fake_dom, 1, 0, sh11, hole(b["pub8"], 0), lag, 2, hp, hp, out10), operands(fake_dom, 1, 0, sh11, pub8, hole(b["lag"], 1), 2, hp, hp, out10),
             operands(fake_dom, 1, 0, sh11, pub8, lag, 2, hp, hp, hole(b["out10"], 9)),
             combine(None, 1, 0, sh14, l1, hp, out2), combine(fake_dom, 1, 0, None, l1, hp, out2), combine(fake_dom, 1, 0, sh14, None, hp, out2),
             combine(fake_dom, 1, 0, sh14, l1, None, out2), combine(fake_dom, 1, 0, sh14, l1, hp, None),
             combine(fake_dom, 1, 0, hole(b["sh14"], 13), l1, hp, out2), combine(fake_dom, 1, 0, sh14, l1, hp, hole(b["out2"], 1))]
    full = [_p(ct), _p(ctz), hp, _p(t1), _p(t2), _p(t3)]
    for k in range(6):
        calls.append(finish(0, n, 1, 0, *(full[:k] + [None] + full[k + 1:])))
    for i, rc in enumerate(calls):
        assert rc == INVALID, (i, rc)
    assert b"NULL" in err()
    # finish: the field, n, and the overlap rules
    for f in (2, 9):
        assert finish(f, n, 1, 0, *full) == INVALID and b"field_of" in err()
    for bad_n in (0, 1, 4, 12, 24, (1 << 27)):
        assert finish(0, bad_n, 1, 0, *full) == INVALID and b"power of two" in err(), bad_n
    big = np.zeros(4 * 2 * (4 * n + 4 * n + 2 * (n + 1) + (n + 6)), dtype=np.uint64)
    w = 8   # words per Rep3 share
    o_ct, o_ctz, o_t1, o_t2, o_t3 = 0, 4 * n * w, 8 * n * w, (9 * n + 1) * w, (10 * n + 2) * w
    at = lambda off: _p(big[off:])
    for args, msg in (((at(o_ct), at(o_ctz), hp, at(o_ct), at(o_t2), at(o_t3)), b"overlaps an input"),             # in place
                      ((at(o_ct), at(o_ctz), hp, at(o_t1 - w), at(o_t2), at(o_t3)), b"overlaps an input"),         # t1 begins inside ctz
                      ((at(o_ct), at(o_ctz), hp, at(o_t1), at(o_t2), at(o_ctz + (3 * n - 6) * w + 1)), b"overlaps an input"),
                      ((at(o_ct), at(o_ctz), hp, at(o_t1), at(o_t2 - w), at(o_t3)), b"two outputs overlap"),       # t2 begins on t1's b9
                      ((at(o_ct), at(o_ctz), hp, at(o_t1), at(o_t3), at(o_t3)), b"two outputs overlap")):
        assert finish(0, n, 1, 0, *args) == INVALID and msg in err(), (msg, err())
    assert finish(0, n, 0, 0, at(o_ct), at(o_ctz), hp, at(o_t1), at(o_t1 + 4 * n), at(o_t3)) == INVALID   # ncomp 1: t1 is n + 1 shares of 4 words


def test_no_device_no_result(hip):
    """Without a device every valid call fails with the no-device error: there is no CPU path."""
    if hip.have_device():
        pytest.skip("a HIP device is present")
    L = hip.lib()
    b = _abi_bufs()
    fake_dom = C.c_void_p(b["host"].ctypes.data)   # not looked into without a device
    hp = _p(b["host"])
    n = 8
    ct, ctz = np.zeros(4 * 2 * 4 * n, dtype=np.uint64), np.zeros(4 * 2 * 4 * n, dtype=np.uint64)
    t1, t2, t3 = (np.zeros(4 * 2 * (n + k), dtype=np.uint64) for k in (1, 1, 6))
    big = np.zeros(4 * 2 * (4 * n + 4 * n + 2 * (n + 1) + (n + 6)), dtype=np.uint64)
    for rc in (L.csh_plonk_quot_blinders_dev(fake_dom, u32(1), u32(2), hp, _ptrs(b["out5"]), None),
               L.csh_plonk_quot_operands_dev(fake_dom, u32(1), u32(1), _ptrs(b["sh11"]), _ptrs(b["pub8"]), _ptrs(b["lag"]), sz(2), hp, hp, _ptrs(b["out10"]), None),
               L.csh_plonk_quot_operands_dev(fake_dom, u32(0), u32(0), _ptrs(b["sh11"]), _ptrs(b["pub8"]), None, sz(0), None, hp, _ptrs(b["out10"]), None),
               L.csh_plonk_quot_combine_dev(fake_dom, u32(0), u32(0), _ptrs(b["sh14"]), _p(b["lag"][0]), hp, _ptrs(b["out2"]), None),
               L.csh_plonk_quot_finish_dev(1, sz(n), u32(1), u32(0), _p(ct), _p(ctz), hp, _p(t1), _p(t2), _p(t3), None),
               L.csh_plonk_quot_finish_dev(1, sz(n), u32(1), u32(0), _p(big), _p(big[32 * n:]), hp, _p(big[64 * n:]), _p(big[72 * n + 8:]),
                                           _p(big[80 * n + 16:]), None)):   # back to back is no overlap
        assert rc == NO_DEVICE
        assert re.search(b"no HIP device|no CPU fallback", L.csh_last_error())


@pytest.mark.parametrize("curve", CURVES)
def test_derived_tables_match_get_z1_z2_z3(hip, curve):
    F = H.FR[curve]
    for n in (8, 16, 1 << 10):
        w_ext = ext_generator(F, n)
        out = np.zeros(4 * 12, dtype=np.uint64)
        rc = hip.lib().csh_selftest_plonk_quot_host(H.CURVE_IDS[curve], 4, _p(H.pack(F, [w_ext])), sz(4 * n), u32(0), u32(0), None, sz(0), None, _ptrs([out]))
        assert rc == 0
        root2 = pow(w_ext, n, F.p)
        assert root2 != 1 and pow(root2, 2, F.p) == F.p - 1
        assert H.unpack(F, out) == R.get_z1(F.p, root2) + R.get_z2(F.p, root2) + R.get_z3(F.p, root2)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("protocol,party", PARTIES)
@pytest.mark.parametrize("n_public", [0, 1, 3])
def test_stages_match_the_restatement(hip, curve, protocol, party, n_public):
    F = H.FR[curve]
    r = H.rng(1000 * protocol + 100 * party + n_public)
    w_ext = ext_generator(F, 8)
    run_all_stages(hip, curve, R.stage_case(F.p, protocol, party, 8, w_ext, n_public, lambda: r.randrange(F.p)), w_ext)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("protocol,party", PARTIES)
@pytest.mark.parametrize("fill", ["p-1", "0"])
def test_stages_at_the_edges_of_the_field(hip, curve, protocol, party, fill):
    """every operand p - 1 (shares, public vectors, challenges, blinders), and every operand 0; bound checks on"""
    F = H.FR[curve]
    v = F.p - 1 if fill == "p-1" else 0
    w_ext = ext_generator(F, 8)
    run_all_stages(hip, curve, R.stage_case(F.p, protocol, party, 8, w_ext, 3, lambda: v), w_ext)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("protocol,party", [(0, 0), (1, 1)])
def test_public_input_sum_over_chunks(hip, curve, protocol, party):
    """two launches' worth of Lagrange vectors with a ragged second one, and three; every term (p - 1)(p - 1); then random terms"""
    F = H.FR[curve]
    w_ext = ext_generator(F, 8)
    for n_public in (16 + 5, 2 * 16 + 1, 16):
        run_all_stages(hip, curve, R.stage_case(F.p, protocol, party, 8, w_ext, n_public, lambda: F.p - 1), w_ext)
    r = H.rng(77)
    run_all_stages(hip, curve, R.stage_case(F.p, protocol, party, 8, w_ext, 16 + 5, lambda: r.randrange(F.p)), w_ext)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("protocol", [0, 1])
@pytest.mark.parametrize("with_rest", [False, True])
def test_division_by_zh_is_an_exact_inverse(hip, curve, protocol, with_rest):
    F, T = H.FR[curve], R.Ops(H.FR[curve].p, protocol, 0)
    for n in (8, 32):
        q, ct, ctz, b9, b10 = R.division_case(F.p, T, n, H.rng(n + protocol), with_rest)
        case = {"T": T, "N": 4 * n, "n": n, "buffer_a": []}
        t1, t2, t3 = _run_host(hip, curve, 3, case, ext_generator(F, n), [_vec(F, ct), _vec(F, ctz)], R.flat([b9, b10]), [n + 1, n + 1, n + 6])
        R.check_division(T, n, q, ct, ctz, b9, b10, t1, t2, t3)
