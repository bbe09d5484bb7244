"""The bytes that the seeded entry points of the host mirror (cog16_*) give for fixed non-zero seeds and given r, s, as sha256 digests
recorded once on the MI355X. All arithmetic is exact field arithmetic and every generator is a ShareRng of a fixed (seed, domain), so the
bytes are deterministic; a digest that moves means a draw order, a domain or an output layout moved. Calls that draw from OS entropy
(seed 0, NULL r / s) are left out. The driver entries run at n = 8, n = 1 and n = 0; a digest of no bytes (the quotient of a constant, the
inverse of nothing) still pins that the call is accepted."""
import ctypes as C
import gzip
import hashlib
import json
import os
import random

import numpy as np
import pytest

from cosnarks_amd import groth16 as g
from oracle import curves as cv
from oracle import groth16 as g16
from tests import helpers as H

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CURVES = ("bn254", "bls12_381")
R, S = 0x1234567890ABCDEF1122334455667788, 0x0FEDCBA987654321
DRIVERS = (g.PLAIN, g.REP3, g.SHAMIR)


def _circuit(curve):
    d = os.path.join(GOLD, "Groth16", curve, "multiplier2")   # the smallest committed circuit: one constraint, domain 4
    return open(os.path.join(d, "circuit.zkey"), "rb").read(), open(os.path.join(d, "witness.wtns"), "rb").read()


def _limbs(curve, seed, n):
    return H.uniform_limbs(H.FR[curve], np.random.RandomState(seed), n)


def _proof(p):
    return json.dumps(p, sort_keys=True).encode()


def _prove_rep3(curve):
    zk, wt = _circuit(curve)
    proof, h = g.prove_rep3(H.CURVE_IDS[curve], zk, wt, seed=41, r=R, s=S, want_h=True, h_elems=4)
    return _proof(proof) + h.tobytes()


def _prove_shamir(curve, n, t, bridge):
    zk, wt = _circuit(curve)
    return _proof(g.prove_shamir(H.CURVE_IDS[curve], zk, wt, n, t, seed=42, r=R, s=S, bridge=bridge))


def _prove_from_shares(curve, protocol, compression):
    zk, wt = _circuit(curve)
    files = g.split_witness(H.CURVE_IDS[curve], protocol, wt, 2, seed=43, compression=compression)
    return _proof(g.prove_from_shares(H.CURVE_IDS[curve], protocol, zk, files, threshold=1, seed=44, r=R, s=S))


def _translate_witness(curve, compression):
    _, wt = _circuit(curve)
    return b"".join(g.translate_witness(H.CURVE_IDS[curve], g.split_witness(H.CURVE_IDS[curve], "rep3", wt, 2, seed=45, compression=compression)))


def _witness_map(curve, reduction):
    F = H.FR[curve]
    A, B, Cm, w = g16.random_r1cs(F, random.Random(46), 2, 5)
    mont = lambda M: [[(F.to_mont(c), i) for c, i in row] for row in M]
    return g.witness_map(H.CURVE_IDS[curve], reduction, True, (mont(A), mont(B), mont(Cm)), 2, H.pack(F, w), seed=47).tobytes()


def _prove_libsnark(shamir):
    """The reference's Penumbra output circuit on BLS12-377 with the key of the restated arkworks generator (tests/helpers.py)."""
    (F, _, _, _, _, _, exp), _, _, pk, _ = H.penumbra_libsnark_key()
    d = os.path.join(GOLD, "Groth16", "bls12_377", "penumbra_output")
    a, b, c, w = (gzip.open(os.path.join(d, n + ".gz"), "rb").read() for n in ("a.bin", "b.bin", "c.bin", "witness.wtns"))
    rl, sl = H.pack(F, [R % F.p], mont=False), H.pack(F, [S], mont=False)
    L = g.glib()
    args = (3, a, C.c_size_t(len(a)), b, C.c_size_t(len(b)), c, C.c_size_t(len(c)), w, C.c_size_t(len(w)), pk, C.c_size_t(len(pk)))
    out = (C.c_uint8 * 512)()
    rs = (rl.ctypes.data_as(C.c_void_p), sl.ctypes.data_as(C.c_void_p), out, C.c_size_t(512))
    if shamir:
        n = L.cog16_prove_libsnark_shamir(*args, 3, 1, C.c_uint64(48), *rs)
        assert n == 384, L.cog16_last_error()
        return bytes(out[:n])
    hs = np.zeros(3 * exp["domain_size"] * 4, dtype=np.uint64)
    n = L.cog16_prove_libsnark_rep3(*args, C.c_uint64(49), *rs, hs.ctypes.data_as(C.c_void_p), C.c_size_t(3 * exp["domain_size"]))
    assert n == 384, L.cog16_last_error()
    return bytes(out[:n]) + hs.tobytes()


def _mle_fold(curve, driver, op):
    polys = [_limbs(curve, 60 + i, 8) for i in range(3 if op == 0 else 1)]
    out = g.driver_mle_fold(H.CURVE_IDS[curve], driver, ("partially_evaluate", "fold_polynomials", "evaluate_mle")[op], polys, _limbs(curve, 59, 3),
                            npub=1 if op == 0 else 0, seed=50)
    return b"".join(x.tobytes() for x in out) if op == 0 else out.tobytes()


def _msm(curve, driver, n):
    G = cv.CURVES[curve][0]
    pts = cv.pack_points(G, H.rand_points(G, n, random.Random(61))) if n else np.zeros(0, dtype=np.uint64)
    return g.driver_msm(H.CURVE_IDS[curve], driver, pts, _limbs(curve, 62, n), seed=51).tobytes()


def _cases():
    E = {}
    for curve in CURVES:
        cid = H.CURVE_IDS[curve]
        add = lambda name, fn, curve=curve: E.__setitem__(curve + "-" + name, fn)
        add("prove_rep3-h", lambda curve=curve: _prove_rep3(curve))
        for n, t, bridge in ((3, 1, False), (5, 2, False), (3, 1, True)):
            add("prove_shamir-%d-%d%s" % (n, t, "-bridge" if bridge else ""), lambda curve=curve, n=n, t=t, bridge=bridge: _prove_shamir(curve, n, t, bridge))
        for protocol, comp in (("rep3", 0), ("rep3", 1), ("rep3", 3), ("shamir", 0)):
            add("prove_from_shares-%s-%d" % (protocol, comp), lambda curve=curve, protocol=protocol, comp=comp: _prove_from_shares(curve, protocol, comp))
        for comp, kind in ((0, "replicated"), (1, "additive")):
            add("translate_witness-" + kind, lambda curve=curve, comp=comp: _translate_witness(curve, comp))
        for driver in DRIVERS:
            for inverse in (False, True):
                add("driver_fft-%d-%s" % (driver, "ifft" if inverse else "fft"), lambda cid=cid, curve=curve, driver=driver, inverse=inverse: g.driver_fft(
                    cid, driver, _limbs(curve, 52, 8), 8, inverse=inverse, seed=53).tobytes())
            for n in (8, 1, 0):
                add("driver_local_mul_vec-%d-n%d" % (driver, n), lambda cid=cid, curve=curve, driver=driver, n=n: g.driver_local_mul_vec(
                    cid, driver, _limbs(curve, 54, n), _limbs(curve, 55, n), seed=56).tobytes())
                add("driver_msm-%d-n%d" % (driver, n), lambda curve=curve, driver=driver, n=n: _msm(curve, driver, n))
            for n in (8, 1):   # n = 0 is refused by every driver, in both forms: "factor_roots: empty polynomial"
                add("driver_factor_roots-%d-n%d" % (driver, n), lambda cid=cid, curve=curve, driver=driver, n=n: g.driver_factor_roots(
                    cid, driver, _limbs(curve, 54, n), _limbs(curve, 55, 1), seed=56).tobytes())
                add("driver_div_by_zerofier-%d-n%d" % (driver, n), lambda cid=cid, curve=curve, driver=driver, n=n: g.driver_factor_roots(
                    cid, driver, _limbs(curve, 54, n), _limbs(curve, 55, 1), seed=56, zerofier=True).tobytes())
            for n in (8, 1, 0):
                add("driver_eval_poly-%d-n%d" % (driver, n), lambda cid=cid, curve=curve, driver=driver, n=n: g.driver_eval_poly(
                    cid, driver, _limbs(curve, 54, n), _limbs(curve, 55, 1), seed=56).tobytes())
                for mode in (0, 1, 2):
                    add("driver_inv_vec-%d-n%d-mode%d" % (driver, n, mode), lambda cid=cid, curve=curve, driver=driver, n=n, mode=mode: g.driver_inv_vec(
                        cid, driver, _limbs(curve, 54, n), seed=57, leaking_zeros=mode == 1, in_place=mode == 2).tobytes())
            add("driver_batched_quotient-%d" % driver, lambda cid=cid, curve=curve, driver=driver: g.driver_batched_quotient(
                cid, driver, [_limbs(curve, 54, 8), _limbs(curve, 55, 3)], _limbs(curve, 63, 2), _limbs(curve, 64, 2), _limbs(curve, 65, 1), seed=58).tobytes())
            for op in (0, 1, 2):
                add("driver_mle_fold-%d-op%d" % (driver, op), lambda curve=curve, driver=driver, op=op: _mle_fold(curve, driver, op))
        for n in (8, 1, 0):
            add("driver_array_prod_mul-n%d" % n, lambda cid=cid, curve=curve, n=n: g.driver_array_prod_mul(
                cid, _limbs(curve, 54, n), _limbs(curve, 55, n), _limbs(curve, 66, n), inv=True).tobytes())
    for curve in CURVES + ("bls12_377",):
        for reduction in (g.CIRCOM_REDUCTION, g.LIBSNARK_REDUCTION):
            E["%s-witness_map-rep3-reduction%d" % (curve, reduction)] = lambda curve=curve, reduction=reduction: _witness_map(curve, reduction)
    E["bls12_377-prove_libsnark_rep3-h"] = lambda: _prove_libsnark(False)
    E["bls12_377-prove_libsnark_shamir-3-1"] = lambda: _prove_libsnark(True)
    return E


CASES = _cases()

SHA256 = {
    "bls12_377-prove_libsnark_rep3-h": "bfec5a269db949d7a9b5d4de02eb0649e9a0ea7dd617e59a711ce99b453d4fde",
    "bls12_377-prove_libsnark_shamir-3-1": "b1f651038e71d5a4357606f077969222656598add14a7446e49ebc099cf6469a",
    "bls12_377-witness_map-rep3-reduction0": "9e359ee65d7cdfe1614d9ee073d17466b8faeac83f54b39275b17800eafe89c5",
    "bls12_377-witness_map-rep3-reduction1": "5ededc1f6151cb42b01271717f5d5e81fa1d54c5ee398b7de5f93d2b73c9de8f",
    "bls12_381-driver_array_prod_mul-n0": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "bls12_381-driver_array_prod_mul-n1": "1ab97989b6325faef53ff6e1405836c23be378cf3cd2f2acc1a26acb82175282",
    "bls12_381-driver_array_prod_mul-n8": "fd31e670ee1f8486385cc2d5a1d93e0899bd18eb6fdf734233e88146dddc30c6",
    "bls12_381-driver_batched_quotient-0": "f2306a9849f652c7ef31b6792cd58a14dc98b77c886b0cd7d241c6fc13f185ff",
    "bls12_381-driver_batched_quotient-1": "a4a3cbeea4c7d7332eca8acf9853f75d41407b2e045e67c4f21ddca0a41f4a25",
    "bls12_381-driver_batched_quotient-2": "c14bc3254127ff3dd02561d43b159814378530e03151522c9e5160dc94f161e1",
    "bls12_381-driver_div_by_zerofier-0-n1": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "bls12_381-driver_div_by_zerofier-0-n8": "b003a38291bfb491dc330f7ba97fee16fb2c13a6dfa7811caeea6bc953074815",
    "bls12_381-driver_div_by_zerofier-1-n1": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "bls12_381-driver_div_by_zerofier-1-n8": "5457980899dca40833899776e2f042d7bac5765ecdad1d2d4fa25c59886da5ef",
    "bls12_381-driver_div_by_zerofier-2-n1": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "bls12_381-driver_div_by_zerofier-2-n8": "0302dac6de4d851d8e2c8facf88e41a724e8308482f044f7f874b17705f6c823",
    "bls12_381-driver_eval_poly-0-n0": "66687aadf862bd776c8fc18b8e9f8e20089714856ee233b3902a591d0d5f2925",
    "bls12_381-driver_eval_poly-0-n1": "f09ae6707c72513afb1ce2afde3dbf65681036fbab519eeacc2ad199efb63031",
    "bls12_381-driver_eval_poly-0-n8": "5fb0445ea26e4f26574a6068c8451b36dbb2b60a5a2f4fc20f6d29ce7761e7c1",
    "bls12_381-driver_eval_poly-1-n0": "5d89f056865052bcb89c910d2d62872e029fb273c3db03f8968a52a41593c1b5",
    "bls12_381-driver_eval_poly-1-n1": "50017551130fa8d626962eb35c59d1c93a4135e060650e6962f133254826e749",
    "bls12_381-driver_eval_poly-1-n8": "c2257c8b828414b5fa54b8562034731e800b0522bb6964a9f5aa419ace90ace5",
    "bls12_381-driver_eval_poly-2-n0": "66687aadf862bd776c8fc18b8e9f8e20089714856ee233b3902a591d0d5f2925",
    "bls12_381-driver_eval_poly-2-n1": "f09ae6707c72513afb1ce2afde3dbf65681036fbab519eeacc2ad199efb63031",
    "bls12_381-driver_eval_poly-2-n8": "5fb0445ea26e4f26574a6068c8451b36dbb2b60a5a2f4fc20f6d29ce7761e7c1",
    "bls12_381-driver_factor_roots-0-n1": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "bls12_381-driver_factor_roots-0-n8": "b003a38291bfb491dc330f7ba97fee16fb2c13a6dfa7811caeea6bc953074815",
    "bls12_381-driver_factor_roots-1-n1": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "bls12_381-driver_factor_roots-1-n8": "5457980899dca40833899776e2f042d7bac5765ecdad1d2d4fa25c59886da5ef",
    "bls12_381-driver_factor_roots-2-n1": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "bls12_381-driver_factor_roots-2-n8": "0302dac6de4d851d8e2c8facf88e41a724e8308482f044f7f874b17705f6c823",
    "bls12_381-driver_fft-0-fft": "8c17f63c43b3f646f9f1b84316cb76107c916e79acc6039f81d932a9ae3b033d",
    "bls12_381-driver_fft-0-ifft": "36efd33ba1eeed3c1a467791b7f5a317069834763d60d5c1c39bb3574c606e4a",
    "bls12_381-driver_fft-1-fft": "2d0bd3d7284827fc0a1909d0d56353548f5ff2555f7debcf8531f65ea3176cad",
    "bls12_381-driver_fft-1-ifft": "565ba8223c22c79970788fd08e29d68c7fc8ef7609531d04577d84fdfeedb5d0",
    "bls12_381-driver_fft-2-fft": "8c17f63c43b3f646f9f1b84316cb76107c916e79acc6039f81d932a9ae3b033d",
    "bls12_381-driver_fft-2-ifft": "36efd33ba1eeed3c1a467791b7f5a317069834763d60d5c1c39bb3574c606e4a",
    "bls12_381-driver_inv_vec-0-n0-mode0": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "bls12_381-driver_inv_vec-0-n0-mode1": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "bls12_381-driver_inv_vec-0-n0-mode2": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "bls12_381-driver_inv_vec-0-n1-mode0": "26a38d8efda156c1b9afdda9af342cfe33a4b1052f90645c0dc53e4418cc63ad",
    "bls12_381-driver_inv_vec-0-n1-mode1": "26a38d8efda156c1b9afdda9af342cfe33a4b1052f90645c0dc53e4418cc63ad",
    "bls12_381-driver_inv_vec-0-n1-mode2": "26a38d8efda156c1b9afdda9af342cfe33a4b1052f90645c0dc53e4418cc63ad",
    "bls12_381-driver_inv_vec-0-n8-mode0": "66e90f43bc9a569c1e8e9b1beaae2f22ea44a735893ad0deaf1ff173fcfa4372",
    "bls12_381-driver_inv_vec-0-n8-mode1": "66e90f43bc9a569c1e8e9b1beaae2f22ea44a735893ad0deaf1ff173fcfa4372",
    "bls12_381-driver_inv_vec-0-n8-mode2": "66e90f43bc9a569c1e8e9b1beaae2f22ea44a735893ad0deaf1ff173fcfa4372",
    "bls12_381-driver_inv_vec-1-n0-mode0": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "bls12_381-driver_inv_vec-1-n0-mode1": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "bls12_381-driver_inv_vec-1-n0-mode2": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "bls12_381-driver_inv_vec-1-n1-mode0": "40dd62fa7358ddf9d4939be71b996f22766e77b826dbdbf861e7203d53c8e390",
    "bls12_381-driver_inv_vec-1-n1-mode1": "40dd62fa7358ddf9d4939be71b996f22766e77b826dbdbf861e7203d53c8e390",
    "bls12_381-driver_inv_vec-1-n1-mode2": "40dd62fa7358ddf9d4939be71b996f22766e77b826dbdbf861e7203d53c8e390",
    "bls12_381-driver_inv_vec-1-n8-mode0": "ac3c4e875454138edf38c246e1623f30a2ee793ee4e3f62a065f304cc99abc50",
    "bls12_381-driver_inv_vec-1-n8-mode1": "ac3c4e875454138edf38c246e1623f30a2ee793ee4e3f62a065f304cc99abc50",
    "bls12_381-driver_inv_vec-1-n8-mode2": "ac3c4e875454138edf38c246e1623f30a2ee793ee4e3f62a065f304cc99abc50",
    "bls12_381-driver_inv_vec-2-n0-mode0": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "bls12_381-driver_inv_vec-2-n0-mode1": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "bls12_381-driver_inv_vec-2-n0-mode2": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "bls12_381-driver_inv_vec-2-n1-mode0": "13f3884813e44ce4f0084d9b60ea16c52d0f833eb76d87c2094df650c9d1c32d",
    "bls12_381-driver_inv_vec-2-n1-mode1": "13f3884813e44ce4f0084d9b60ea16c52d0f833eb76d87c2094df650c9d1c32d",
    "bls12_381-driver_inv_vec-2-n1-mode2": "13f3884813e44ce4f0084d9b60ea16c52d0f833eb76d87c2094df650c9d1c32d",
    "bls12_381-driver_inv_vec-2-n8-mode0": "0d1032aa872f87ad858ecae3127883b33dd830be247012911e4215ee189057da",
    "bls12_381-driver_inv_vec-2-n8-mode1": "0d1032aa872f87ad858ecae3127883b33dd830be247012911e4215ee189057da",
    "bls12_381-driver_inv_vec-2-n8-mode2": "0d1032aa872f87ad858ecae3127883b33dd830be247012911e4215ee189057da",
    "bls12_381-driver_local_mul_vec-0-n0": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "bls12_381-driver_local_mul_vec-0-n1": "9e30906de2d6239cc4290e40d4f13d95aaa53e9bcd0c26c9bbb06980be54c67a",
    "bls12_381-driver_local_mul_vec-0-n8": "0cfad913f47b29453cfc35cd46aabcf98058f8f2c39e492e70ad08a604b803b7",
    "bls12_381-driver_local_mul_vec-1-n0": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "bls12_381-driver_local_mul_vec-1-n1": "1ce5be36694c9d78eb72dd30a69f90d566eef06859a21f2ccdda110fea429266",
    "bls12_381-driver_local_mul_vec-1-n8": "04552c2fec489b78ba8854bc44ed02a1a39bed3124f11df52a3f4a4bb0442d81",
    "bls12_381-driver_local_mul_vec-2-n0": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "bls12_381-driver_local_mul_vec-2-n1": "9e30906de2d6239cc4290e40d4f13d95aaa53e9bcd0c26c9bbb06980be54c67a",
    "bls12_381-driver_local_mul_vec-2-n8": "0cfad913f47b29453cfc35cd46aabcf98058f8f2c39e492e70ad08a604b803b7",
    "bls12_381-driver_mle_fold-0-op0": "32587d42128aeea7497bcad7155a180affa1276bf492cf8a162049f6c198cd9b",
    "bls12_381-driver_mle_fold-0-op1": "c5ec8be10fc290ca324e24848e101e8bda31a22c7a8214dc22b6d444de975c4a",
    "bls12_381-driver_mle_fold-0-op2": "c109f3b7754c99e14f29d4226bde2dea5a08346d26bf0d930be17c970f110b88",
    "bls12_381-driver_mle_fold-1-op0": "8594b2820284adda34842fd74ccf50d5e709dd730110a26af8ae8aef5d28820f",
    "bls12_381-driver_mle_fold-1-op1": "f37b2bbf6662d9d0f80caef729d2b472677215073b7dcdbc83209077d5cc0caf",
    "bls12_381-driver_mle_fold-1-op2": "07ab8e68dd9d5519d907511930caa907f5bb38888968a3b0710776e2cbedca52",
    "bls12_381-driver_mle_fold-2-op0": "88363fc93fbd0ad2c3bef9716ae528792f96412ae234907eef52d083a06e9bc3",
    "bls12_381-driver_mle_fold-2-op1": "152778c4853c8b4b2a2110cf788dc00fdcf390230cc33964f91413f33c7f5826",
    "bls12_381-driver_mle_fold-2-op2": "7d9b3f9078c5f2003e914125dec75cc2fe9d5b4a3f3b1e8a90187dc99094ae1f",
    "bls12_381-driver_msm-0-n0": "2ea9ab9198d1638007400cd2c3bef1cc745b864b76011a0e1bc52180ac6452d4",
    "bls12_381-driver_msm-0-n1": "b425790966c88ff3d40adbd791bae7d991b002a92d548c98d9de7b30ebfa942b",
    "bls12_381-driver_msm-0-n8": "c8c9ea2b47539e342aeefb2d0b8d6aa2a5648ba9de4d2fe2baca8efb5145517d",
    "bls12_381-driver_msm-1-n0": "1a0295f4bf5986c5f74eca9153a6a4cb10b073a01a76ba4a457fd862c78966a4",
    "bls12_381-driver_msm-1-n1": "ed2855d233849624e0769b2dd54c28f83333844de605cbfa5652098b4743d234",
    "bls12_381-driver_msm-1-n8": "93d50f2263abdbc0fec0280d76057fd33b1ca873dfaa7fcc113dc36389ed85d8",
    "bls12_381-driver_msm-2-n0": "2ea9ab9198d1638007400cd2c3bef1cc745b864b76011a0e1bc52180ac6452d4",
    "bls12_381-driver_msm-2-n1": "b425790966c88ff3d40adbd791bae7d991b002a92d548c98d9de7b30ebfa942b",
    "bls12_381-driver_msm-2-n8": "c8c9ea2b47539e342aeefb2d0b8d6aa2a5648ba9de4d2fe2baca8efb5145517d",
    "bls12_381-prove_from_shares-rep3-0": "7574c07867e3c6a356b6f1a4dc5f4341362c15d9a7577fcd1795b8e6e95e9c67",
    "bls12_381-prove_from_shares-rep3-1": "7574c07867e3c6a356b6f1a4dc5f4341362c15d9a7577fcd1795b8e6e95e9c67",
    "bls12_381-prove_from_shares-rep3-3": "7574c07867e3c6a356b6f1a4dc5f4341362c15d9a7577fcd1795b8e6e95e9c67",
    "bls12_381-prove_from_shares-shamir-0": "7574c07867e3c6a356b6f1a4dc5f4341362c15d9a7577fcd1795b8e6e95e9c67",
    "bls12_381-prove_rep3-h": "f4d890f5c724acb559874d44c517de8a32c90dca37641b36dffd662c917967f2",
    "bls12_381-prove_shamir-3-1": "7574c07867e3c6a356b6f1a4dc5f4341362c15d9a7577fcd1795b8e6e95e9c67",
    "bls12_381-prove_shamir-3-1-bridge": "7574c07867e3c6a356b6f1a4dc5f4341362c15d9a7577fcd1795b8e6e95e9c67",
    "bls12_381-prove_shamir-5-2": "7574c07867e3c6a356b6f1a4dc5f4341362c15d9a7577fcd1795b8e6e95e9c67",
    "bls12_381-translate_witness-additive": "022dead1ffea40d77aea4dee17f17c83665dac852834a166ea54c4889d33f67d",
    "bls12_381-translate_witness-replicated": "022dead1ffea40d77aea4dee17f17c83665dac852834a166ea54c4889d33f67d",
    "bls12_381-witness_map-rep3-reduction0": "ad4aa807dd2af933aa6788209c2098bc85c7a132aa1a4e1a3237ad34ecd09332",
    "bls12_381-witness_map-rep3-reduction1": "356a917b05e08f715abd2a21f221a56f20cfec07e3097319e316697693d1692d",
    "bn254-driver_array_prod_mul-n0": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "bn254-driver_array_prod_mul-n1": "604fab7091bda65913f1a4052f27164bd44e2652264adc4398a13e5a6add5240",
    "bn254-driver_array_prod_mul-n8": "6d101e8ada4c739dfde90df186e6124025a955a678c47c49fe73ff7e5700479a",
    "bn254-driver_batched_quotient-0": "dafa8a2f6425a5a59b5e65f742f62a92a55c4267bbc42c31cd0af36d17562cef",
    "bn254-driver_batched_quotient-1": "60443e20faceaf8667bb0157707a3c3bbaa61278db3454d7aaed1774ac2dc9e9",
    "bn254-driver_batched_quotient-2": "e8ed0b4fe56e15a8aee4933bc7ed193e68d599caa437496b58fb4b89ab75d6dd",
    "bn254-driver_div_by_zerofier-0-n1": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "bn254-driver_div_by_zerofier-0-n8": "e72bafa7aac82cac268fa41157c9da86aa6272443b2fdc9154c5e4e1c7aded05",
    "bn254-driver_div_by_zerofier-1-n1": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "bn254-driver_div_by_zerofier-1-n8": "bf04becc0cfcc03bac32b7325f22a0f16933dba5bf757d56a4acb250296ae242",
    "bn254-driver_div_by_zerofier-2-n1": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "bn254-driver_div_by_zerofier-2-n8": "8898d2c8395bd7524c2f11285afacdd0cd657470749e4dac2d799179f0ef96e2",
    "bn254-driver_eval_poly-0-n0": "66687aadf862bd776c8fc18b8e9f8e20089714856ee233b3902a591d0d5f2925",
    "bn254-driver_eval_poly-0-n1": "f09ae6707c72513afb1ce2afde3dbf65681036fbab519eeacc2ad199efb63031",
    "bn254-driver_eval_poly-0-n8": "70c50cfdb29e60c4a34d4c2fde2e2d2005942775d73e89a6d64b1f9a2fc5bc6c",
    "bn254-driver_eval_poly-1-n0": "5d89f056865052bcb89c910d2d62872e029fb273c3db03f8968a52a41593c1b5",
    "bn254-driver_eval_poly-1-n1": "ba6ce0455f7ed2088eecc78c25948aaac18fc829ab48e0606dac990501509894",
    "bn254-driver_eval_poly-1-n8": "c1fa4c9198137f64e13fd4235f9e17ccc856e8dbaadd6008a2961645e2b73e57",
    "bn254-driver_eval_poly-2-n0": "66687aadf862bd776c8fc18b8e9f8e20089714856ee233b3902a591d0d5f2925",
    "bn254-driver_eval_poly-2-n1": "f09ae6707c72513afb1ce2afde3dbf65681036fbab519eeacc2ad199efb63031",
    "bn254-driver_eval_poly-2-n8": "70c50cfdb29e60c4a34d4c2fde2e2d2005942775d73e89a6d64b1f9a2fc5bc6c",
    "bn254-driver_factor_roots-0-n1": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "bn254-driver_factor_roots-0-n8": "e72bafa7aac82cac268fa41157c9da86aa6272443b2fdc9154c5e4e1c7aded05",
    "bn254-driver_factor_roots-1-n1": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "bn254-driver_factor_roots-1-n8": "bf04becc0cfcc03bac32b7325f22a0f16933dba5bf757d56a4acb250296ae242",
    "bn254-driver_factor_roots-2-n1": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "bn254-driver_factor_roots-2-n8": "8898d2c8395bd7524c2f11285afacdd0cd657470749e4dac2d799179f0ef96e2",
    "bn254-driver_fft-0-fft": "b49b31225d320bc9ebb627095986f4993b01f1c67f20f4f4b55db57d466ae810",
    "bn254-driver_fft-0-ifft": "2700f3ac759dc9113c9aa08a1358ab2948ae6b57fb8b73560b8d032273cbbbbc",
    "bn254-driver_fft-1-fft": "096f782210413994b40cf211207de43cebf0fb8bbf94a70c6ecff053532fe363",
    "bn254-driver_fft-1-ifft": "9f4c214a1f5e46b1f6ce2bdffcf17b15be6e13946adc8e0107f4110ceff0e24c",
    "bn254-driver_fft-2-fft": "b49b31225d320bc9ebb627095986f4993b01f1c67f20f4f4b55db57d466ae810",
    "bn254-driver_fft-2-ifft": "2700f3ac759dc9113c9aa08a1358ab2948ae6b57fb8b73560b8d032273cbbbbc",
    "bn254-driver_inv_vec-0-n0-mode0": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "bn254-driver_inv_vec-0-n0-mode1": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "bn254-driver_inv_vec-0-n0-mode2": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "bn254-driver_inv_vec-0-n1-mode0": "3897a6743e49f787b09b67f6f0960a3322754b084203cd8912b48c662e541786",
    "bn254-driver_inv_vec-0-n1-mode1": "3897a6743e49f787b09b67f6f0960a3322754b084203cd8912b48c662e541786",
    "bn254-driver_inv_vec-0-n1-mode2": "3897a6743e49f787b09b67f6f0960a3322754b084203cd8912b48c662e541786",
    "bn254-driver_inv_vec-0-n8-mode0": "f347b97c4cd604ca8f8a284955c9b70e458675fa96ca9fb22e897b97aae78ddf",
    "bn254-driver_inv_vec-0-n8-mode1": "f347b97c4cd604ca8f8a284955c9b70e458675fa96ca9fb22e897b97aae78ddf",
    "bn254-driver_inv_vec-0-n8-mode2": "f347b97c4cd604ca8f8a284955c9b70e458675fa96ca9fb22e897b97aae78ddf",
    "bn254-driver_inv_vec-1-n0-mode0": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "bn254-driver_inv_vec-1-n0-mode1": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "bn254-driver_inv_vec-1-n0-mode2": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "bn254-driver_inv_vec-1-n1-mode0": "f3b25f101c5a3f7577818dbaac6f66ccef40e3ad6c32e18eecf12c6172072464",
    "bn254-driver_inv_vec-1-n1-mode1": "f3b25f101c5a3f7577818dbaac6f66ccef40e3ad6c32e18eecf12c6172072464",
    "bn254-driver_inv_vec-1-n1-mode2": "f3b25f101c5a3f7577818dbaac6f66ccef40e3ad6c32e18eecf12c6172072464",
    "bn254-driver_inv_vec-1-n8-mode0": "1b56e05241426bbdcdcac94eda5175c4493e5e6ac687d11563fd1d4501ad991a",
    "bn254-driver_inv_vec-1-n8-mode1": "1b56e05241426bbdcdcac94eda5175c4493e5e6ac687d11563fd1d4501ad991a",
    "bn254-driver_inv_vec-1-n8-mode2": "1b56e05241426bbdcdcac94eda5175c4493e5e6ac687d11563fd1d4501ad991a",
    "bn254-driver_inv_vec-2-n0-mode0": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "bn254-driver_inv_vec-2-n0-mode1": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "bn254-driver_inv_vec-2-n0-mode2": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "bn254-driver_inv_vec-2-n1-mode0": "ef17ad132ce238aae14ce8fda2a0291599e45bcb9f8f6ff93f98b622036f6fce",
    "bn254-driver_inv_vec-2-n1-mode1": "ef17ad132ce238aae14ce8fda2a0291599e45bcb9f8f6ff93f98b622036f6fce",
    "bn254-driver_inv_vec-2-n1-mode2": "ef17ad132ce238aae14ce8fda2a0291599e45bcb9f8f6ff93f98b622036f6fce",
    "bn254-driver_inv_vec-2-n8-mode0": "ed03c777147694aefc478176b1d5eee2b9daed6692f77ede60ba2b635ba4315e",
    "bn254-driver_inv_vec-2-n8-mode1": "ed03c777147694aefc478176b1d5eee2b9daed6692f77ede60ba2b635ba4315e",
    "bn254-driver_inv_vec-2-n8-mode2": "ed03c777147694aefc478176b1d5eee2b9daed6692f77ede60ba2b635ba4315e",
    "bn254-driver_local_mul_vec-0-n0": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "bn254-driver_local_mul_vec-0-n1": "1df339c9931e03365f1871e9d1efa32fad2d129a533f7bdf48ea469483cbfc7e",
    "bn254-driver_local_mul_vec-0-n8": "c607731748e33e81deece6653db2c7ac0a2cf14cb20190e24c860c9eb1a3c3cb",
    "bn254-driver_local_mul_vec-1-n0": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "bn254-driver_local_mul_vec-1-n1": "00762ea6cc143dd88acfa476941f3a3d5811f0a25ba855b26c293580d8b02d57",
    "bn254-driver_local_mul_vec-1-n8": "eee4a6a6c9df6bf39a7d0a83eda5a8a2a1c2474ad4d863adf19d28ca8d0b725a",
    "bn254-driver_local_mul_vec-2-n0": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "bn254-driver_local_mul_vec-2-n1": "1df339c9931e03365f1871e9d1efa32fad2d129a533f7bdf48ea469483cbfc7e",
    "bn254-driver_local_mul_vec-2-n8": "c607731748e33e81deece6653db2c7ac0a2cf14cb20190e24c860c9eb1a3c3cb",
    "bn254-driver_mle_fold-0-op0": "8d1a80d21cd654e46b1ae8c8601b53f64d40b15875aa99271521808dd95d4d37",
    "bn254-driver_mle_fold-0-op1": "e47caa39f2ccf9f304f91deee27102ae4e7696a353cec00134a11f1bb6c0e3b8",
    "bn254-driver_mle_fold-0-op2": "c7c53ab977dd7c3b13d2b51068da822cf7c3742b19f18b9f5d1202e2f6725533",
    "bn254-driver_mle_fold-1-op0": "030d8834eb3d84f426c39f8bd2dc897702ed8bcc9141e80750c7ddea77dd4946",
    "bn254-driver_mle_fold-1-op1": "ff6a99861b9242e8ed3917f20364e510b113abde0d189b6cee62a0e29d05fac0",
    "bn254-driver_mle_fold-1-op2": "16f8f9dbd9752fe34277964f4ccbcaf637195a73c63101dce1ac1c03b08cc3c9",
    "bn254-driver_mle_fold-2-op0": "20575b6127bab66851acdc841f435d133c28c458fc312a0bba5007d1c4079271",
    "bn254-driver_mle_fold-2-op1": "944e1a1a72b9f4430519cbb3e88f76b6a1ea9d058649308e39c8e44d0f5ac4e2",
    "bn254-driver_mle_fold-2-op2": "ba70dad6df92e5386dd71963bd3b35bcd2f6aa353b6dece76adb7a04f40af6a6",
    "bn254-driver_msm-0-n0": "f5a5fd42d16a20302798ef6ed309979b43003d2320d9f0e8ea9831a92759fb4b",
    "bn254-driver_msm-0-n1": "554ce226dca99d4b637550b9ce306400b5af552cb3ef03ca7e8119f5968a3397",
    "bn254-driver_msm-0-n8": "286fa30e2ac255a8c366abb56ced896bbbf651ac541f2e45d0e348ebf0e17f38",
    "bn254-driver_msm-1-n0": "a1a4f5721c1c4610af7f71078f3a68c330536d679803b0e0507ee8dc10c5dfca",
    "bn254-driver_msm-1-n1": "80820239a0db2c5f91a69eaba7424ea5e398b9539bd98a60fa7a85ae231276a4",
    "bn254-driver_msm-1-n8": "816677769e7d48b19f186b6916b853ca8e0b8e8f7143bed813c4098ef178094a",
    "bn254-driver_msm-2-n0": "f5a5fd42d16a20302798ef6ed309979b43003d2320d9f0e8ea9831a92759fb4b",
    "bn254-driver_msm-2-n1": "554ce226dca99d4b637550b9ce306400b5af552cb3ef03ca7e8119f5968a3397",
    "bn254-driver_msm-2-n8": "286fa30e2ac255a8c366abb56ced896bbbf651ac541f2e45d0e348ebf0e17f38",
    "bn254-prove_from_shares-rep3-0": "a41d7c8c12a1f65194686c36264859ab0fe36a3829303f3b8fb8c5a6eadca7af",
    "bn254-prove_from_shares-rep3-1": "a41d7c8c12a1f65194686c36264859ab0fe36a3829303f3b8fb8c5a6eadca7af",
    "bn254-prove_from_shares-rep3-3": "a41d7c8c12a1f65194686c36264859ab0fe36a3829303f3b8fb8c5a6eadca7af",
    "bn254-prove_from_shares-shamir-0": "a41d7c8c12a1f65194686c36264859ab0fe36a3829303f3b8fb8c5a6eadca7af",
    "bn254-prove_rep3-h": "d9bae2684321ee94d129cdfc18f71cd1213e835ac0b269a19c49225e425bab6c",
    "bn254-prove_shamir-3-1": "a41d7c8c12a1f65194686c36264859ab0fe36a3829303f3b8fb8c5a6eadca7af",
    "bn254-prove_shamir-3-1-bridge": "a41d7c8c12a1f65194686c36264859ab0fe36a3829303f3b8fb8c5a6eadca7af",
    "bn254-prove_shamir-5-2": "a41d7c8c12a1f65194686c36264859ab0fe36a3829303f3b8fb8c5a6eadca7af",
    "bn254-translate_witness-additive": "5aa8377b987091bd407dcb31a54a6224ec05d874defa5c9604b1598e9eec112a",
    "bn254-translate_witness-replicated": "5aa8377b987091bd407dcb31a54a6224ec05d874defa5c9604b1598e9eec112a",
    "bn254-witness_map-rep3-reduction0": "bc1ef54d1cedbbf8fc7d74b671012228531c6600fb76842b00c16508af141028",
    "bn254-witness_map-rep3-reduction1": "1d05a8a02b202ca1eac4eba727e3257d7dc14d21589259c7cc005345033c8b29",
}


def test_every_case_has_a_digest():
    assert sorted(CASES) == sorted(SHA256)


@pytest.mark.parametrize("name", sorted(SHA256))
def test_seeded_bytes(gpu, name):
    assert hashlib.sha256(CASES[name]()).hexdigest() == SHA256[name]
