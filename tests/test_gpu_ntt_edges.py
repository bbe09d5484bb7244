"""The NTT pass kernels on structured worst-case inputs (tests/ntt_edge_cases.py), through the public API, bit-exact.

The lazy signed 9 x 29-bit field fails only at the corners of its range; random inputs never get there. Every family -- zeros,
constants, characters (exact zeros by cancellation at every stage), deltas (one operand of every butterfly zero), the edge mix, stored
words with all-ones limbs -- runs through ifft_in_to_out, fft_out_to_in, fft and ifft of every pass form; the result must be canonical
and equal the closed form (the mixes: the oracle -- oracle.ntt.Domain up to 2^13, the C restatement above; the CPU module
test_ntt_edge_cases_cpu.py ties the closed forms to both). No tolerance anywhere.

Shapes: (tune ntt_variant, logn, components per entry) with the pass list (s0, k, cb) the planner gives them today -- each kernel path
at its smallest size. Nothing here asserts the plan; whoever changes the planner finds here which shape was meant for which path.

  variant        logn       ncomp  plan                                    what it reaches
  1 and 2        1          1, 2   (0,1,0)                                 below radix-4: one radix-2 stage, unit twiddle
  1 and 2        2          1, 2   (0,2,0)                                 round4_unit alone / two radix-2 stages
  1 and 2        3          1      (0,3,0)                                 round4_unit + left-over radix-2 stage (last in DIT, local stage 0 in DIF)
  1 and 2        4, 5       1      one pass                                round4_unit + general round4 (+ odd stage)
  1 and 2        8          1, 2   (0,8,0) / (0,7,0),(7,1,6)               full default tile; with shares the first strided pass
  1 and 2        9, 10, 12  1      (0,8,0) + (8,k,cb), k = 1, 2, 4         strided pass: k = 1 is radix-2 also under variant 1, k = 2, 4 general round4 with cb > 0
  0x101, 0x102   11         1      (0,11,0)                                deepest tile: 11 stages between canonicalisations
  0x101, 0x102   10         2      (0,10,0)                                the same with two components
  0x101, 0x102   13         1      (0,11,0),(11,2,9)                       deep tile + strided radix-4 pass
  0x441, 0x442   14         1      (0,8,0),(8,3,5),(11,3,5)                three passes at the smallest size that has them
  0x441, 0x442   13         2      (0,7,0),(7,3,4),(10,3,4)                three passes, shares
  2, ntt_lazy=0  3, 8, 12   1      --                                      the 32-bit CIOS pass (kept for A/B runs) on the same families
  0 (default)    20         1      (0,11,0),(11,9,2)                       default radix-4 choice and tile; two-tone families from numpy.tile

(variant bit 0 forces the radix-4 pass, bit 1 the radix-2 pass; bits 8-10 = 1 force 2^11-element tiles, = 4 2^8-element tiles; bits
4-6 = 4 force 8-entry runs.) BN254 runs every row; BLS12-381 and BLS12-377 (other top limbs: other fold_top reciprocals and R'/p
headroom) the rows with logn 2, 3, 8, 11 (0x101, 0x102) and 14 (0x441, 0x442).

The fused pair kernel (k_ntt_pass_r4<.., PAIR>) is only reached through groth16_h: h of family inputs, with the fused pass forced at
every size and with the two-launch form, against a Python reference built from the oracle's transforms (ntt_edge_cases.h_plain /
h_rep3): logn 2, 3, 8, 11 plain and Rep3 (random and all-zero masks), 12 plain; BN254, plus BLS12-377 at logn 8."""
import numpy as np
import pytest

from oracle import ntt
from tests import helpers as H
from tests import ntt_edge_cases as E

pytestmark = pytest.mark.gpu

_TABLE = [   # (variants, logn, component counts)
    ((1, 2), 1, (1, 2)), ((1, 2), 2, (1, 2)), ((1, 2), 3, (1,)), ((1, 2), 4, (1,)), ((1, 2), 5, (1,)), ((1, 2), 8, (1, 2)),
    ((1, 2), 9, (1,)), ((1, 2), 10, (1,)), ((1, 2), 12, (1,)),
    ((0x101, 0x102), 11, (1,)), ((0x101, 0x102), 10, (2,)), ((0x101, 0x102), 13, (1,)),
    ((0x441, 0x442), 14, (1,)), ((0x441, 0x442), 13, (2,)),
]
_OTHER_FIELD_ROWS = {((1, 2), 2), ((1, 2), 3), ((1, 2), 8), ((0x101, 0x102), 11), ((0x441, 0x442), 14)}


def _rows():
    out = []
    for curve in ("bn254", "bls12_381", "bls12_377"):
        for variants, logn, ncomps in _TABLE:
            if curve != "bn254" and (variants, logn) not in _OTHER_FIELD_ROWS:
                continue
            for v in variants:
                out.append(pytest.param(curve, v, logn, ncomps, id="%s-%#x-2^%d" % (curve, v, logn)))
    return out


def _gen(F, logn):
    return ntt.roots_of_unity(F)[1][logn]


@pytest.fixture(scope="module")
def packed():
    """Inputs and expectations, computed once per (field, size) and never modified (the bindings copy what they are handed)."""
    return E.packed_families


_ENTRIES = ("ifft_in_to_out", "fft_out_to_in", "fft", "ifft")


def _run_families(gpu, packed, curve, logn, ncomps, ctx):
    F = H.FR[curve]
    n = 1 << logn
    pk = packed(curve, logn)
    dg = gpu.Domain(H.CURVE_IDS[curve], logn, H.pack(F, [_gen(F, logn)]))
    try:
        for ncomp in ncomps:
            if ncomp == 1:
                for c, io in pk.cases:
                    for entry in _ENTRIES:
                        vin, want = io[entry]
                        got = getattr(dg, entry)(vin)
                        H.assert_canonical(F, got)
                        assert np.array_equal(got.reshape(n, 4), want), (ctx, c.name, entry)
            else:   # share vectors {a, b} per entry: the two components carry different families
                for (ca, ioa), (cb, iob) in pk.pairs:
                    for entry in _ENTRIES:
                        vin = np.stack([ioa[entry][0], iob[entry][0]], axis=1)
                        got = getattr(dg, entry)(vin, ncomp=2).reshape(n, 2, 4)
                        H.assert_canonical(F, got)
                        assert np.array_equal(got[:, 0], ioa[entry][1]), (ctx, "component a", ca.name, cb.name, entry)
                        assert np.array_equal(got[:, 1], iob[entry][1]), (ctx, "component b", ca.name, cb.name, entry)
    finally:
        dg.free()


@pytest.mark.parametrize("curve,variant,logn,ncomps", _rows())
def test_ntt_edge_families_every_lazy_pass_form(gpu, packed, curve, variant, logn, ncomps):
    """Every row of the module's shape table but the last two, every family, four entry points, plain and share vectors."""
    with gpu.tuned(ntt_variant=variant):
        _run_families(gpu, packed, curve, logn, ncomps, (curve, hex(variant), logn))


@pytest.mark.parametrize("logn", [3, 8, 12])
def test_ntt_edge_families_32bit_pass(gpu, packed, logn):
    """The 32-bit CIOS pass (tune ntt_lazy = 0, kept for A/B runs) on the same families."""
    with gpu.tuned(ntt_variant=2, ntt_lazy=0):
        _run_families(gpu, packed, "bn254", logn, (1,), ("bn254", "32-bit pass", logn))


def test_ntt_two_tone_families_default_plan_2p20(gpu):
    """Default plan at 2^20 (radix-4 by default, 2^11-element tile, one strided pass of 9 stages): zeros, constants, the character
    j = n/2 (alternating +c, -c) and the saturated-limb word alternating with stored 0 and stored p - 1 -- all of them two-tone vectors
    (A on even, B on odd indices) built with numpy.tile; closed forms only (ntt_edge_cases.two_tone_closed_form)."""
    F = H.FR["bn254"]
    logn = 20
    n = 1 << logn
    p = F.p
    sat = E.saturated_value(F)
    tones = [("zeros", 0, 0)] + [("const " + cn, c, c) for cn, c in E.constants(F)] + [("char n/2 " + cn, c, p - c) for cn, c in E.constants(F)]
    tones += [("sat, 0", sat, 0), ("sat, stored p-1", sat, F.from_mont(p - 1))]
    dg = gpu.Domain(H.CURVE_IDS["bn254"], logn, H.pack(F, [_gen(F, logn)]))
    try:
        for name, A, B in tones:
            wa, wb = H.pack(F, [A]).reshape(1, 4), H.pack(F, [B]).reshape(1, 4)
            alternating = np.tile(np.concatenate([wa, wb]), (n // 2, 1))
            halves = np.concatenate([np.tile(wa, (n // 2, 1)), np.tile(wb, (n // 2, 1))])
            inv, fwd = E.two_tone_closed_form(F, logn, A, B)

            def expect(entries):
                out = np.zeros((n, 4), dtype=np.uint64)
                for i, v in entries:
                    out[i] = H.pack(F, [v])
                return out
            inv_nat = [(ntt.bitrev(i, logn), v) for i, v in inv]
            for entry, vin, want in (("ifft_in_to_out", alternating, expect(inv)), ("fft_out_to_in", halves, expect(fwd)),
                                     ("fft", alternating, expect(fwd)), ("ifft", alternating, expect(inv_nat))):
                got = getattr(dg, entry)(vin)
                H.assert_canonical(F, got)
                assert np.array_equal(got.reshape(n, 4), want), (name, entry)
    finally:
        dg.free()


# ---- the fused pair kernel, through groth16_h ---------------------------------------------------------------------------------------
def _h_input_pairs(F, logn, g):
    """(name, X, Y): constant x character; character x character with j1 + j2 = n; saturated-limb alternation x edge mix; zeros x random"""
    n = 1 << logn
    p = F.p
    sat = E.saturated_value(F)
    j1 = 1 if n == 2 else H.rng(logn).randrange(1, n)
    return [
        ("const sat x char n-1 p-1", E.constant_case(F, logn, "sat", sat).inv_in, E.character_case(F, logn, g, n - 1, "p-1", p - 1).inv_in),
        ("char %d (p-1)/2 x char %d sat" % (j1, n - j1), E.character_case(F, logn, g, j1, "", (p - 1) // 2).inv_in,
         E.character_case(F, logn, g, n - j1, "", sat).inv_in),
        ("sat mix x edge mix", E.saturated_mix_case(F, logn).inv_in, E.edge_mix_case(F, logn, 31 + logn).inv_in),
        ("zeros x random", [0] * n, H.rand_elems(F, n, H.rng(77 + logn))),
    ]


@pytest.fixture(scope="module")
def h_cases():
    """Inputs and reference h per (field, size), computed once: [(name, protocol, a, b, mask_c, mask_ab, want)] as packed arrays.
    Rep3: a = {X, Y}, b = {Y, X} per entry, with random masks and with all-zero masks."""
    memo = {}

    def get(curve, logn, rep3):
        key = (curve, logn, rep3)
        if key in memo:
            return memo[key]
        F = H.FR[curve]
        n = 1 << logn
        g = _gen(F, logn)
        shift = ntt.roots_of_unity(F)[1][logn + 1]
        ce = E.make_coset_eval(F, ntt.Domain(F, n, g), shift)
        r = H.rng(900 + logn)
        out = []
        for name, X, Y in _h_input_pairs(F, logn, g):
            out.append((name, 0, H.pack(F, X), H.pack(F, Y), None, None, H.pack(F, E.h_plain(F, ce, X, Y))))
            if not rep3:
                continue
            a, b = E.interleave(X, Y), E.interleave(Y, X)
            for mname, mc, mab in (("random masks", H.rand_elems(F, n, r), H.rand_elems(F, n, r)), ("zero masks", [0] * n, [0] * n)):
                out.append((name + ", Rep3, " + mname, 1, H.pack_shares(F, a), H.pack_shares(F, b), H.pack(F, mc), H.pack(F, mab),
                            H.pack(F, E.h_rep3(F, ce, a, b, mc, mab))))
        memo[key] = (H.pack(F, [shift]), out)
        return memo[key]
    return get


@pytest.mark.parametrize("curve,logn,rep3", [("bn254", 2, True), ("bn254", 3, True), ("bn254", 8, True), ("bn254", 11, True),
                                             ("bn254", 12, False), ("bls12_377", 8, True)])
def test_h_on_edge_families_fused_pair_and_two_launches(gpu, h_cases, curve, logn, rep3):
    """groth16_h with the fused tile pass forced (PAIR kernel: DIF rounds, scale-table product, canonical_wide().pack() -> unpack
    hand-over in LDS, DIT rounds) and as two launches, against the oracle-built reference. The constant and character inputs put
    exact zeros through the scale-table multiplication and the hand-over."""
    F = H.FR[curve]
    shift, cases = h_cases(curve, logn, rep3)
    dom = gpu.Domain(H.CURVE_IDS[curve], logn, H.pack(F, [_gen(F, logn)]))
    try:
        for form, knobs in (("pair", {"ntt_pair": 1, "ntt_pair_min_log": 0}), ("two launches", {"ntt_pair": 0})):
            with gpu.tuned(**knobs):
                for name, protocol, a, b, mc, mab, want in cases:
                    got = gpu.bindings.groth16_h(dom, shift, protocol, a, b, mc, mab)
                    H.assert_canonical(F, got)
                    assert np.array_equal(got, want), (curve, logn, form, name)
    finally:
        dom.free()
