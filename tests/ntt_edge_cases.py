"""Structured worst-case inputs of the NTT with closed-form transforms (plain functions shared by the CPU and the device tests).

The lazy signed 9 x 29-bit field of the NTT kernels can only fail at the corners of its range: butterfly outputs that are exact
multiples of p (as lazy values 0, +-p, 2p, ...), operands at the top of the field, stored words whose 29-bit limbs are all ones.
Uniformly random inputs meet none of them; the families below meet them at every stage.

Conventions are those of oracle/ntt.py (g = group generator of order n = 2^logn, br = ntt.bitrev):
    ifft_in_to_out: natural-order values v_k            -> coefficient i = (1/n) sum_k v_k g^(-ik), stored at br(i)
    fft_out_to_in : coefficients c_i, stored at br(i)   -> X_k = sum_i c_i g^(ik), natural order

Families (c = element value, from constants(F)):
    zeros          all zero in, all zero out
    const          inverse: [c] * n -> c at index 0;                     forward: [c] * n -> n c at index 0
    char j         inverse: v_k = c g^(jk) -> c at index br(j);          forward: c_i = c g^(-ji) -> n c at index j
                   (j = n/2 is the alternating +c, -c vector: exact zeros by cancellation at every stage, non-trivial twiddles)
    delta j        inverse: c at index j -> coefficient i = c g^(-ij)/n; forward: c at index br(j) -> X_k = c g^(jk)
                   (one operand of every butterfly is zero)
    edge mix       seeded draws from H.edge_elems(F) mod p plus (p +- 1)/2; no closed form
    sat mix        stored words 2^252 - 1 (limbs 0..7 of the 29-bit slicing all ones, a canonical residue of all three scalar
                   fields), 0 and p - 1 in turn (period 3, so every butterfly of every stage pairs two different ones); no closed form
    two-tone A, B  (the large-size stand-in of the mixes, built with numpy.tile in the device test) v_k = A for even k, B for odd k,
                   = (A+B)/2 + (A-B)/2 (-1)^k: inverse -> (A+B)/2 at index 0 and (A-B)/2 at index br(n/2) = 1; forward (input in
                   bit-reversed storage: first half A, second half B) -> n (A+B)/2 at index 0, n (A-B)/2 at index n/2
"""
import collections
import functools

import numpy as np

from oracle import cbridge, mpc, ntt
from tests import helpers as H

SATURATED_WORD = (1 << 252) - 1   # stored 256-bit word: limbs 0..7 of the 9 x 29-bit slicing are all ones

# name, family, and per direction the input and the closed-form output as lists of Python ints (None: no closed form)
Case = collections.namedtuple("Case", "name family inv_in inv_out fwd_in fwd_out")


def saturated_value(F):
    """the element whose stored (Montgomery) word is SATURATED_WORD"""
    assert SATURATED_WORD < F.p
    return F.from_mont(SATURATED_WORD)


def constants(F):
    return [("1", 1), ("p-1", F.p - 1), ("(p-1)/2", (F.p - 1) // 2), ("sat", saturated_value(F))]


def character_indices(n, seed):
    """{1, n/2, n-1, one seeded random j}, without repeats, each < n"""
    js = []
    for j in (1, n // 2, n - 1, H.rng(seed).randrange(n)):
        if 0 <= j < n and j not in js:
            js.append(j)
    return js


def delta_indices(n):
    js = []
    for j in (0, 1, n - 1):
        if j < n and j not in js:
            js.append(j)
    return js


def _powers(F, base, n, c):
    """[c base^k for k < n]"""
    out, cur = [], c % F.p
    for _ in range(n):
        out.append(cur)
        cur = cur * base % F.p
    return out


def _sparse(n, entries):
    v = [0] * n
    for i, x in entries:
        v[i] = x
    return v


def constant_case(F, logn, cname, c):
    n = 1 << logn
    return Case("const c=%s" % cname, "const", [c] * n, _sparse(n, [(0, c)]), [c] * n, _sparse(n, [(0, n * c % F.p)]))


def character_case(F, logn, g, j, cname, c):
    n = 1 << logn
    p = F.p
    inv_in = _powers(F, pow(g, j, p), n, c)
    inv_out = _sparse(n, [(ntt.bitrev(j, logn), c)])
    fwd_in = ntt.bit_reverse(_powers(F, pow(g, -j, p), n, c))
    fwd_out = _sparse(n, [(j, n * c % p)])
    return Case("char j=%d c=%s" % (j, cname), "char", inv_in, inv_out, fwd_in, fwd_out)


def delta_case(F, logn, g, j, cname, c):
    n = 1 << logn
    p = F.p
    inv_in = _sparse(n, [(j, c)])
    inv_out = ntt.bit_reverse(_powers(F, pow(g, -j, p), n, c * pow(n, -1, p)))
    fwd_in = _sparse(n, [(ntt.bitrev(j, logn), c)])
    fwd_out = _powers(F, pow(g, j, p), n, c)
    return Case("delta j=%d c=%s" % (j, cname), "delta", inv_in, inv_out, fwd_in, fwd_out)


def edge_mix_case(F, logn, seed):
    n = 1 << logn
    pool = [v % F.p for v in H.edge_elems(F)] + [(F.p + 1) // 2, (F.p - 1) // 2]
    r = H.rng(seed)
    v = [r.choice(pool) for _ in range(n)]
    return Case("edge mix", "edge", v, None, v, None)


def saturated_mix_case(F, logn):
    n = 1 << logn
    vals = [saturated_value(F), 0, F.from_mont(F.p - 1)]
    v = [vals[i % 3] for i in range(n)]
    return Case("sat mix", "sat", v, None, v, None)


def two_tone_closed_form(F, logn, A, B):
    """-> (inverse entries, forward entries) as [(index, value)] of the outputs of the two-tone family; every other output is zero.
    The inverse input is [A, B, A, B, ...], the forward input [A] * (n/2) + [B] * (n/2)."""
    n = 1 << logn
    p = F.p
    half = pow(2, -1, p)
    s, d = (A + B) * half % p, (A - B) * half % p
    if logn == 0:
        return [(0, A % p)], [(0, A % p)]
    return [(0, s), (1, d)], [(0, n * s % p), (n // 2, n * d % p)]


def two_tone_case(F, logn, name, A, B):
    n = 1 << logn
    inv, fwd = two_tone_closed_form(F, logn, A, B)
    return Case("two-tone " + name, "tone", [A, B] * (n // 2), _sparse(n, inv), [A] * (n // 2) + [B] * (n // 2), _sparse(n, fwd))


def families(F, logn, g, seed=0):
    """Every family at size 2^logn (logn >= 1) with generator g: the list of Cases."""
    n = 1 << logn
    cs = constants(F)
    sat = saturated_value(F)
    out = [Case("zeros", "zeros", [0] * n, [0] * n, [0] * n, [0] * n)]
    out += [constant_case(F, logn, cn, c) for cn, c in cs]
    out += [character_case(F, logn, g, j, cn, c) for j in character_indices(n, 1000 * logn + seed) for cn, c in cs]
    out += [delta_case(F, logn, g, j, cn, c) for j in delta_indices(n) for cn, c in cs]
    out.append(edge_mix_case(F, logn, 2000 * logn + seed))
    out.append(saturated_mix_case(F, logn))
    out.append(two_tone_case(F, logn, "sat, 0", sat, 0))
    out.append(two_tone_case(F, logn, "sat, stored p-1", sat, F.from_mont(F.p - 1)))
    return out


def share_pairs(cases):
    """Rep3 share vectors (two components per entry): component a carries case i, component b case i + k, with the rotation k chosen
    so that the two always belong to DIFFERENT families -- a component mix-up cannot cancel. -> [(case_a, case_b)]"""
    m = len(cases)
    for k in range(1, m):
        if all(cases[i].family != cases[(i + k) % m].family for i in range(m)):
            return [(cases[i], cases[(i + k) % m]) for i in range(m)]
    raise AssertionError("no rotation separates the families")


def interleave(a, b):
    """component vectors -> the share vector [(a_0, b_0), ...]"""
    return list(zip(a, b))


# ---- the families as C-ABI limb arrays, with the oracle's transforms where there is no closed form ------------------------------------
def bitrev_perm(logn):
    idx = np.arange(1 << logn, dtype=np.uint32)
    rev = np.zeros_like(idx)
    for b in range(logn):
        rev |= ((idx >> b) & 1) << (logn - 1 - b)
    return rev


class PackedFamilies:
    """One (field, size): every family packed once -- inputs and expected outputs of the four entry points as (n, 4) u64 arrays.
    fft takes the bit reversal of fft_out_to_in's input, ifft returns the bit reversal of ifft_in_to_out's output. The mixes take their
    expectation from oracle.ntt.Domain up to 2^13 and from the C restatement above. `extra`: further Cases without a closed form."""

    def __init__(self, curve, logn, extra=()):
        F = H.FR[curve]
        g = ntt.roots_of_unity(F)[1][logn]
        n = 1 << logn
        cid = H.CURVE_IDS[curve]
        rev = bitrev_perm(logn)
        pk = lambda v: H.pack(F, v).reshape(n, 4)
        self.cases = []
        dom = ntt.Domain(F, n, g) if logn <= 13 else None
        for c in families(F, logn, g) + list(extra):
            inv_in, fwd_in = pk(c.inv_in), pk(c.fwd_in)
            if c.inv_out is not None:
                inv_out, fwd_out = pk(c.inv_out), pk(c.fwd_out)
            elif dom is not None:
                inv_out, fwd_out = pk(dom.ifft_in_to_out(c.inv_in)), pk(dom.fft_out_to_in(c.fwd_in))
            else:
                pg = H.pack(F, [g])
                inv_out = cbridge.ntt(cid, inv_in, logn, pg, dif=True).reshape(n, 4)
                fwd_out = cbridge.ntt(cid, fwd_in, logn, pg, dif=False).reshape(n, 4)
            # per entry point: (input, expected output)
            self.cases.append((c, {"ifft_in_to_out": (inv_in, inv_out), "fft_out_to_in": (fwd_in, fwd_out),
                                   "fft": (fwd_in[rev], fwd_out), "ifft": (inv_in, inv_out[rev])}))
        by_case = {id(c): (c, io) for c, io in self.cases}
        self.pairs = [(by_case[id(ca)], by_case[id(cb)]) for ca, cb in share_pairs([c for c, _ in self.cases])]


@functools.lru_cache(maxsize=None)
def packed_families(curve, logn):
    """PackedFamilies(curve, logn) plus one uniformly random vector (family "random"), built once per process; read-only by agreement"""
    F = H.FR[curve]
    v = H.rand_elems(F, 1 << logn, H.rng(4000 + logn))
    return PackedFamilies(curve, logn, extra=[Case("random", "random", v, None, v, None)])


# ---- h of the Groth16 witness map (CircomReduction tail), restated from the oracle's transforms ----------------------------------
def make_coset_eval(F, dom, shift):
    """-> ce(v) = fft_out_to_in(coset_table . ifft_in_to_out(v)), table = ntt.bit_reversed_coset_table(shift); results are kept per
    input vector (the plain and the Rep3 form of one test case evaluate the same component vectors)"""
    table = ntt.bit_reversed_coset_table(F, shift, dom.size)
    memo = {}

    def ce(v):
        key = tuple(v)
        if key not in memo:
            memo[key] = dom.fft_out_to_in([x * t % F.p for x, t in zip(dom.ifft_in_to_out(list(v)), table)])
        return memo[key]
    return ce


def h_plain(F, ce, a, b):
    """h = ce(a) ce(b) - ce(a . b)"""
    p = F.p
    ab = ce([x * y % p for x, y in zip(a, b)])
    return [(x * y - z) % p for x, y, z in zip(ce(a), ce(b), ab)]


def h_rep3(F, ce, a, b, mask_c, mask_ab):
    """The Rep3 form (a, b: share vectors [(a_i, b_i)]): ab = local_mul(a, b) + mask_c as one component; the share vectors are
    transformed component-wise; h = local_mul(ce(a), ce(b)) + mask_ab - ce(ab)."""
    ab = ce(mpc.rep3_local_mul_vec(F, a, b, mask_c))
    ce2 = lambda s: interleave(ce([x[0] for x in s]), ce([x[1] for x in s]))
    prod = mpc.rep3_local_mul_vec(F, ce2(a), ce2(b), mask_ab)
    return [(x - z) % F.p for x, z in zip(prod, ab)]
