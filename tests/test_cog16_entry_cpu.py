"""What the C entry points of the host mirror (libcosnarks_groth16.so, cog16_*) answer to a bad argument, as a table of literal expectations:
the return value and a piece of cog16_last_error(). Every entry that takes a curve is called with the id 99 and with each of the ids 2
(Grumpkin) and 3 (BLS12-377) it does not serve; the other rows are the refusals that come before any device use. Which argument an entry
looks at first is part of the ABI: the bench entries look at `iters`, cog16_driver_mle_fold at `op`, cog16_prove_libsnark_shamir at the
party range before the curve. The second table pins the bytes of cog16_split_witness (host only) for a fixed seed, i.e. the draw order of
the Rep3 and Shamir sharers (ShareRng domains 1 and 2)."""
import ctypes as C
import hashlib
import os
import re

import numpy as np
import pytest

from cosnarks_amd import groth16 as g

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sz, u64 = C.c_size_t, C.c_uint64
WTNS = open(os.path.join(GOLD, "Groth16", "bn254", "multiplier2", "witness.wtns"), "rb").read()   # the smallest committed witness: 4 values
UNKNOWN = (-1, b"unknown curve")


class Bufs:
    """Host memory for every call below: a refused call reads and writes none of it."""

    def __init__(self):
        self.a, self.b, self.c, self.out = (np.zeros(4 * 64, dtype=np.uint64) for _ in range(4))
        self.blob = bytes(64)                                  # stands for a zkey, a key, a matrix blob, a share file
        self.files = (C.c_char_p * 3)(self.blob, self.blob, self.blob)
        self.lens = (sz * 3)(64, 64, 64)
        self.sizes = (sz * 8)()
        self.ms, self.ok, self.devices = (C.c_double * 32)(), C.c_int(0), (C.c_int * 3)(0, 0, 0)
        self.handle = C.c_void_p(0)
        self.variant, self.npub, self.nwit = C.c_uint32(0), sz(0), sz(0)
        self.text = C.create_string_buffer(4096)
        self.bytes_out = (C.c_uint8 * 4096)()
        self.csr = ((C.POINTER(C.c_uint64) * 3)(), (C.POINTER(C.c_uint32) * 3)(), (C.POINTER(C.c_uint64) * 3)())


def _p(x):
    return x.ctypes.data_as(C.c_void_p)


def _entry_points(L, B):
    """name -> call(curve, **what is wrong besides): valid arguments (8 elements, three parties, threshold 1) around the one under test."""
    a, b, c, out = _p(B.a), _p(B.b), _p(B.c), _p(B.out)
    blob, n64 = B.blob, sz(64)
    mats = (blob, n64, blob, n64, blob, n64)
    L.cog16_rep3_wire.restype = C.c_long
    E = {
        "cog16_driver_fft": lambda cv: L.cog16_driver_fft(cv, 0, 0, 1, a, sz(8), sz(8), u64(1), out),
        "cog16_driver_local_mul_vec": lambda cv: L.cog16_driver_local_mul_vec(cv, 0, a, b, sz(8), u64(1), out),
        "cog16_driver_eval_poly": lambda cv: L.cog16_driver_eval_poly(cv, 0, a, sz(8), b, u64(1), out),
        "cog16_driver_factor_roots": lambda cv: L.cog16_driver_factor_roots(cv, 0, 0, a, sz(8), b, u64(1), out),
        "cog16_driver_batched_quotient": lambda cv: L.cog16_driver_batched_quotient(cv, 0, a, (sz * 1)(8), sz(1), b, c, b, u64(1), out),
        "cog16_driver_mle_fold": lambda cv, op=0, npub=0: L.cog16_driver_mle_fold(cv, 0, op, a, sz(npub), sz(1), sz(8), b, sz(3), 0, u64(1), out),
        "cog16_plonk_compute_t": lambda cv: L.cog16_plonk_compute_t(cv, sz(8), sz(0), a, b, out),
        "cog16_driver_inv_vec": lambda cv: L.cog16_driver_inv_vec(cv, 0, a, sz(8), u64(1), 0, out),
        "cog16_driver_array_prod_mul": lambda cv: L.cog16_driver_array_prod_mul(cv, 0, a, b, c, sz(8), out),
        "cog16_driver_msm": lambda cv: L.cog16_driver_msm(cv, 0, a, sz(2), b, sz(2), u64(1), out),
        "cog16_libsnark_from_files": lambda cv: L.cog16_libsnark_from_files(cv, *mats, blob, n64, sz(1), out, sz(64)),
        "cog16_prove_libsnark": lambda cv: L.cog16_prove_libsnark(cv, *mats, blob, n64, blob, n64, a, b, B.bytes_out, sz(4096), None, sz(0)),
        "cog16_prove_libsnark_shamir": lambda cv, parties=3: L.cog16_prove_libsnark_shamir(cv, *mats, blob, n64, blob, n64, parties, 1, u64(1), a, b,
                                                                                             B.bytes_out, sz(4096)),
        "cog16_prove_libsnark_rep3": lambda cv: L.cog16_prove_libsnark_rep3(cv, *mats, blob, n64, blob, n64, u64(1), a, b, B.bytes_out, sz(4096),
                                                                             None, sz(0)),
        "cog16_ark_roundtrip": lambda cv: L.cog16_ark_roundtrip(cv, 0, a, sz(8), B.bytes_out, sz(4096)),
        "cog16_rep3_wire": lambda cv: L.cog16_rep3_wire(cv, 0, 0, a, sz(8), B.bytes_out, sz(4096)),
        "cog16_witness_map": lambda cv: L.cog16_witness_map(cv, 0, 0, *B.csr, sz(1), sz(1), a, sz(2), u64(1), out, sz(64)),
        "cog16_split_witness": lambda cv, protocol=0, compression=0, threshold=1, parties=3, cap=4096: L.cog16_split_witness(
            cv, protocol, WTNS, sz(len(WTNS)), sz(2), compression, threshold, parties, u64(7), B.bytes_out, sz(cap), B.sizes),
        "cog16_share_file_roundtrip": lambda cv, protocol=0: L.cog16_share_file_roundtrip(cv, protocol, blob, n64, B.bytes_out, sz(4096),
                                                                                         C.byref(B.variant), C.byref(B.npub), C.byref(B.nwit)),
        "cog16_public_inputs_json": lambda cv, protocol=0: L.cog16_public_inputs_json(cv, protocol, blob, n64, B.text, sz(4096)),
        "cog16_prove_from_shares": lambda cv: L.cog16_prove_from_shares(cv, 0, blob, n64, B.files, B.lens, 3, 1, u64(1), a, b, B.text, sz(4096)),
        "cog16_translate_witness": lambda cv: L.cog16_translate_witness(cv, B.files, B.lens, B.bytes_out, sz(4096), B.sizes),
        "cog16_prove_shamir": lambda cv: L.cog16_prove_shamir(cv, blob, n64, WTNS, sz(len(WTNS)), 3, 1, u64(1), a, b, 0, B.text, sz(4096)),
        "cog16_bench_synthetic": lambda cv, iters=1: L.cog16_bench_synthetic(cv, 10, iters, B.ms, C.byref(B.ok), 0),
        "cog16_bench_synthetic2": lambda cv, iters=1: L.cog16_bench_synthetic2(cv, 10, iters, B.ms, C.byref(B.ok), 0, None),
        "cog16_bench_synthetic3": lambda cv, iters=1: L.cog16_bench_synthetic3(cv, 10, iters, B.ms, C.byref(B.ok), 0, None, None),
        "cog16_bench_synthetic4": lambda cv, iters=1: L.cog16_bench_synthetic4(cv, 10, iters, B.ms, C.byref(B.ok), 0, None, None, None, None),
        "cog16_bench_rep3_party_per_gpu": lambda cv, iters=1: L.cog16_bench_rep3_party_per_gpu(cv, 10, iters, B.devices, B.ms),
        "cog16_rep3_rand_selftest": lambda cv: L.cog16_rep3_rand_selftest(cv, bytes(96), sz(4), sz(4), out, B.bytes_out),
        "cog16_synth_open": lambda cv: L.cog16_synth_open(cv, 10, C.byref(B.handle)),
        "cog16_prove_plain": lambda cv: L.cog16_prove_plain(cv, blob, n64, WTNS, sz(len(WTNS)), a, b, B.text, sz(4096), None, sz(0)),
        "cog16_prove_rep3": lambda cv: L.cog16_prove_rep3(cv, blob, n64, WTNS, sz(len(WTNS)), u64(1), a, b, B.text, sz(4096), None, sz(0)),
        # no curve argument
        "cog16_synth_prove": lambda cv: L.cog16_synth_prove(None, None, None),
        "cog16_synth_check": lambda cv: L.cog16_synth_check(None, C.byref(B.ok)),
    }
    return E


# the curves an entry serves beside 0 (BN254) and 1 (BLS12-381)
ALSO_SERVES = {"cog16_driver_msm": (2,), "cog16_libsnark_from_files": (3,), "cog16_prove_libsnark": (3,), "cog16_prove_libsnark_shamir": (3,),
               "cog16_prove_libsnark_rep3": (3,), "cog16_witness_map": (3,)}
NO_CURVE = ("cog16_synth_prove", "cog16_synth_check")
N_WITH_CURVE = 32
N_CURVE_ROWS = 3 * N_WITH_CURVE - len(ALSO_SERVES)     # 90: an id of 99 for each, and each of 2 and 3 where it is not served

# (entry, keyword arguments besides a valid curve 0) -> (return value, piece of the message)
OTHER_ROWS = [
    ("cog16_driver_mle_fold", {"op": 3}, (-1, b"mle_fold: op 0 .. 2; ops 1 and 2 take one shared polynomial")),
    ("cog16_driver_mle_fold", {"op": 1, "npub": 1}, (-1, b"mle_fold: op 0 .. 2; ops 1 and 2 take one shared polynomial")),
    ("cog16_prove_libsnark_shamir", {"parties": 2}, (-1, b"num_parties / threshold out of range")),
    ("cog16_bench_synthetic", {"iters": 0}, (-1, b"cog16_bench_synthetic: iters < 1")),
    ("cog16_bench_synthetic2", {"iters": 0}, (-1, b"cog16_bench_synthetic: iters < 1")),
    ("cog16_bench_synthetic3", {"iters": 0}, (-1, b"cog16_bench_synthetic: iters < 1")),
    ("cog16_bench_synthetic4", {"iters": 0}, (-1, b"cog16_bench_synthetic: iters < 1")),
    ("cog16_bench_rep3_party_per_gpu", {"iters": 0}, (-1, b"cog16_bench_rep3_party_per_gpu: bad arguments")),
    ("cog16_synth_prove", {}, (-1, b"cog16_synth_prove: NULL handle")),
    ("cog16_synth_check", {}, (-1, b"cog16_synth_check: NULL argument")),
    ("cog16_split_witness", {"protocol": 2}, (-1, b"protocol must be 0 (Rep3) or 1 (Shamir)")),
    ("cog16_share_file_roundtrip", {"protocol": 2}, (-1, b"protocol must be 0 (Rep3) or 1 (Shamir)")),
    ("cog16_public_inputs_json", {"protocol": 2}, (-1, b"protocol must be 0 (Rep3) or 1 (Shamir)")),
    ("cog16_split_witness", {"compression": 4}, (-1, b"compression must be 0 (none), 1 (half shares), 2 (seeded shares) or 3 (seeded half shares)")),
    ("cog16_split_witness", {"protocol": 1, "threshold": 1, "parties": 2}, (-1, b"num_parties must be at least 2 * threshold + 1")),
    ("cog16_split_witness", {"cap": 0}, (-1, b"output buffer too small")),
    # the bench entries look at `iters` before the curve
    ("cog16_bench_synthetic4", {"iters": 0, "curve": 99}, (-1, b"cog16_bench_synthetic: iters < 1")),
    ("cog16_bench_rep3_party_per_gpu", {"iters": 0, "curve": 99}, (-1, b"cog16_bench_rep3_party_per_gpu: bad arguments")),
    ("cog16_driver_mle_fold", {"op": 3, "curve": 99}, (-1, b"mle_fold: op 0 .. 2; ops 1 and 2 take one shared polynomial")),
    ("cog16_prove_libsnark_shamir", {"parties": 2, "curve": 99}, (-1, b"num_parties / threshold out of range")),
]


def _curve_rows(E):
    return [(name, cv) for name in sorted(E) if name not in NO_CURVE for cv in (99, 2, 3) if cv not in ALSO_SERVES.get(name, ())]


def actual_rows(L):
    """Every row as the library answers it now: [(label, return value, message)]."""
    E = _entry_points(L, Bufs())
    got = [((name, {"curve": cv}), E[name](cv), L.cog16_last_error()) for name, cv in _curve_rows(E)]
    for name, kw, _ in OTHER_ROWS:
        kw2 = dict(kw)
        got.append(((name, kw), E[name](kw2.pop("curve", 0), **kw2), L.cog16_last_error()))
    return got


# exported entries that take no curve and are not in the table: nothing to dispatch on (what they refuse is in the tests of their features)
NOT_IN_THE_TABLE = ("cog16_last_error", "cog16_set_trait_path", "cog16_get_trait_path", "cog16_synth_close", "cog16_placement_plan",
                    "cog16_set_prover_devices", "cog16_set_prover_devices_mode")


def test_every_exported_entry_is_accounted_for():
    """The names in the built library's dynamic string table: each is in the table above or in NOT_IN_THE_TABLE, so a new entry cannot
    go without rows unnoticed."""
    E = _entry_points(g.glib(), Bufs())
    assert len([n for n in E if n not in NO_CURVE]) == N_WITH_CURVE and len(_curve_rows(E)) == N_CURVE_ROWS
    blob = open(g.glib()._name, "rb").read()
    exported = set(m.decode() for m in re.findall(rb"\0(cog16_[a-z0-9_]+)(?=\0)", blob))
    assert exported == set(E) | set(NOT_IN_THE_TABLE)


def test_refusals():
    L = g.glib()
    rows = actual_rows(L)
    assert len(rows) == N_CURVE_ROWS + len(OTHER_ROWS)
    for (name, kw), rc, msg in rows[:N_CURVE_ROWS]:
        assert (rc, UNKNOWN[1] in msg) == (UNKNOWN[0], True), (name, kw, rc, msg)
    for ((name, kw), rc, msg), (_, _, (want_rc, want_msg)) in zip(rows[N_CURVE_ROWS:], OTHER_ROWS):
        assert rc == want_rc and want_msg in msg, (name, kw, rc, msg)


# sha256 of the files cog16_split_witness writes, one after the other, for the witness above with num_inputs = 2 and seed 0x5eed
SPLIT_SHA256 = {
    (0, 'rep3', 0, 1, 3): "85bd9ec752c0dee755de712d98873a9233c7c9ea762c5c66c32c749ba0c238b3",
    (0, 'rep3', 1, 1, 3): "20766e7d78dd7a2a39e876e524e20953f19e69942ff3bc7ecca265a7e5349aa7",
    (0, 'rep3', 2, 1, 3): "595d473cfc9ce02200ddfd957d1d5a83f1b1743727ddce7f1465a03cf84538c7",
    (0, 'rep3', 3, 1, 3): "8d1d116cfd2eb42265fba328888e443d3bad485322d9c761353ee02e65e27833",
    (1, 'rep3', 0, 1, 3): "73f213c1720248e143943385c9e897cdc16c09d5412853545c95b0aaad1b17c1",
    (1, 'rep3', 1, 1, 3): "45b35d7442919ef50d0dbf8dbda7b7c0f74e107448cb5bc09482417561eeea9d",
    (1, 'rep3', 2, 1, 3): "e4101ac6751e972d35a7ecd5dcfe4afef2f5b58b58b390ed0c6a66c8aa2848b3",
    (1, 'rep3', 3, 1, 3): "6d81382fca11159bb8d66b318ba235bdc9cf1e5218fed2606d05692bc286cfcc",
    (0, 'shamir', 0, 1, 3): "018cdc414bab5203333375aebe55014ec594c5554f67d5f96413c4f10658f7d3",
    (0, 'shamir', 0, 2, 5): "b5abb9a806acbf93335cad4b4b1eb4e3bca0469ba68fc07dde6defe309687e86",
    (1, 'shamir', 0, 1, 3): "acbfb1434a3ab5a4cd1a4b67310831ca290e64edd145e7d8bfac9d856713dff9",
    (1, 'shamir', 0, 2, 5): "db588ff075f00ed08e6348cb3641f392fe94bc4bb5cb58fd97b7ad9309513010",
}


def split_digest(curve, protocol, compression, threshold, parties):
    files = g.split_witness(curve, protocol, WTNS if curve == 0 else WTNS_381, 2, seed=0x5EED, compression=compression, threshold=threshold,
                            num_parties=parties)
    return hashlib.sha256(b"".join(files)).hexdigest()


WTNS_381 = open(os.path.join(GOLD, "Groth16", "bls12_381", "multiplier2", "witness.wtns"), "rb").read()
SPLIT_CASES = [(cv, "rep3", comp, 1, 3) for cv in (0, 1) for comp in range(4)] + [(cv, "shamir", 0, t, n) for cv in (0, 1) for t, n in ((1, 3), (2, 5))]


@pytest.mark.parametrize("case", SPLIT_CASES, ids=lambda c: "-".join(map(str, c)))
def test_split_witness_bytes_for_a_fixed_seed(case):
    assert split_digest(*case) == SPLIT_SHA256[case]
