"""Shared test helpers: seeded inputs and conversions between oracle ints and C-ABI limb arrays."""
import functools
import random

import numpy as np

from oracle import curves as cv
from oracle import fields as fl

FIELD_IDS = {"bn254.Fq": 0, "bn254.Fr": 1, "bls12_381.Fq": 2, "bls12_381.Fr": 3, "bls12_377.Fq": 4, "bls12_377.Fr": 5}
CURVE_IDS = {"bn254": 0, "bls12_381": 1, "grumpkin": 2, "bls12_377": 3}
FR = {"bn254": fl.BN254_FR, "bls12_381": fl.BLS381_FR, "grumpkin": fl.BN254_FQ, "bls12_377": fl.BLS377_FR}   # scalar field of each curve


def rng(seed):
    return random.Random(seed)


def rand_elems(F, n, r):
    return [r.randrange(F.p) for _ in range(n)]


def edge_elems(F):
    return [0, 1, 2, F.p - 1, F.p - 2, (F.p - 1) // 2, (1 << 64) - 1, 1 << 64, F.Rmod, F.R2]


def pack(F, xs, mont=True):
    return fl.pack(F, xs, mont).reshape(-1)


def uniform_limbs(F, rs, n):
    """n field elements of F uniform in [0, p) as (n, 4) u64 limbs (used raw: any value < p is a valid Montgomery encoding). Seeded by
    the numpy RandomState `rs` and vectorised: p.bit_length() random bits per value, values >= p redrawn -- the whole field, including
    its top (on BLS12-381 Fr three quarters of the values are >= 2^253)."""
    assert F.nlimbs == 4
    bits = F.p.bit_length()
    top = np.uint64((1 << (bits - 192)) - 1)
    pl = [np.uint64((F.p >> (64 * i)) & (2**64 - 1)) for i in range(4)]
    out = np.empty((n, 4), dtype=np.uint64)
    todo = np.arange(n)
    while todo.size:
        v = rs.randint(0, 2**64, size=(todo.size, 4), dtype=np.uint64)
        v[:, 3] &= top
        lt, eq = np.zeros(todo.size, dtype=bool), np.ones(todo.size, dtype=bool)
        for i in (3, 2, 1, 0):                      # v < p, most significant limb first
            lt |= eq & (v[:, i] < pl[i])
            eq &= v[:, i] == pl[i]
        out[todo[lt]] = v[lt]
        todo = todo[~lt]
    return out


def unpack(F, arr, mont=True, lenient=False):
    """C-ABI limbs -> ints. Strict by default: every raw word value must be < p (the library's contract: canonical arkworks
    Montgomery form, or canonical integers with mont=False); a lazy value x + p would otherwise decode to the right residue.
    lenient=True only for a documented non-canonical value, with a comment saying why."""
    if not lenient:
        assert_canonical(F, arr)
    return fl.unpack(F, arr, mont)


def assert_canonical(F, arr):
    """Vectorised strict check without decoding (large vectors compared byte for byte elsewhere): every raw word value < p."""
    a = np.ascontiguousarray(arr, dtype="<u8").reshape(-1, F.nlimbs)
    bad = _noncanonical_rows(F, a)
    if bad.size:
        i = int(bad[0])
        raise AssertionError("non-canonical field element at index %d: raw word value %#x >= p (%#x); %d of %d values non-canonical"
                             % (i, int.from_bytes(a[i].tobytes(), "little"), F.p, bad.size, a.shape[0]))


def _noncanonical_rows(F, a):
    """Row indices of a (n, nlimbs) u64 array whose value is >= F.p (vectorised, most significant limb first)."""
    ge, eq = np.zeros(a.shape[0], dtype=bool), np.ones(a.shape[0], dtype=bool)
    for i in reversed(range(F.nlimbs)):
        pi = np.uint64((F.p >> (64 * i)) & (2**64 - 1))
        ge |= eq & (a[:, i] > pi)
        eq &= a[:, i] == pi
    return np.nonzero(ge | eq)[0]


def pack_shares(F, shares):
    """[(a, b)] -> AoS limbs {a, b} per entry."""
    flat = []
    for a, b in shares:
        flat += [a, b]
    return pack(F, flat)


def unpack_shares(F, arr, lenient=False):
    v = unpack(F, arr, lenient=lenient)
    return list(zip(v[0::2], v[1::2]))


def rand_points(curve: cv.Curve, n, r, with_inf=False):
    """n points = random multiples of the generator (in the prime-order subgroup)."""
    pts = []
    base = curve.mul(curve.gen, r.randrange(1, curve.order))
    step = curve.mul(curve.gen, r.randrange(1, curve.order))
    cur = base
    for i in range(n):
        pts.append(cur)
        cur = curve.add(cur, step)
    if with_inf and n >= 4:
        pts[1] = None
        pts[n // 2] = None
    return pts


def known_points(G, n, r):
    """n points with known discrete logarithms: (points, scalars), pts[i] = scalars[i] * G.gen."""
    a, b = r.randrange(1, G.order), r.randrange(1, G.order)
    cur, step = G.mul(G.gen, a), G.mul(G.gen, b)
    pts, sc = [], []
    for i in range(n):
        pts.append(cur)
        sc.append((a + i * b) % G.order)
        cur = G.add(cur, step)
    return pts, sc


def xyzz_to_affine(G, arr, n):
    """n XYZZ points in arkworks words -> oracle affine points; checks the canonical encoding and ZZ^3 == ZZZ^2."""
    F = G.F
    out = []
    for i, (X, Y, ZZ, ZZZ) in enumerate(cv.unpack_points(G, arr, ncoords=4, strict=True)):
        if F.is_zero(ZZ):
            out.append(None)
            continue
        assert F.eq(F.mul(F.sqr(ZZ), ZZ), F.sqr(ZZZ)), "point %d: ZZ^3 != ZZZ^2" % i
        out.append((F.mul(X, F.inv(ZZ)), F.mul(Y, F.inv(ZZZ))))
    return out


def jac_to_affine(curve: cv.Curve, limbs):
    """C-ABI Jacobian output -> oracle affine point. Strict: every coordinate component must be < q (canonical Montgomery form)."""
    (X, Y, Z), = cv.unpack_points(curve, np.asarray(limbs), ncoords=3, strict=True)
    return curve.to_affine((X, Y, Z))


def load_penumbra_fixture():
    """tests/golden/Groth16/bls12_377/penumbra_output (made by tests/golden/make_golden_penumbra.py from the reference's own
    LibSnarkReduction test data): -> (F, A, B, C, public, witness, expected dict)."""
    import gzip
    import json
    import os
    from oracle import arkfmt
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "Groth16", "bls12_377", "penumbra_output")
    rd = lambda n: gzip.open(os.path.join(d, n + ".gz"), "rb").read()
    F = fl.BLS377_FR
    A, B, Cm = (arkfmt.parse_matrix(rd(n)) for n in ["a.bin", "b.bin", "c.bin"])
    prime, w = arkfmt.parse_wtns_positional(rd("witness.wtns"))
    assert prime == F.p
    exp = json.load(open(os.path.join(d, "expected.json")))
    ni = arkfmt.vk_num_instance_variables(rd("circuit.vk"), 96, 192)
    assert ni == exp["num_instance_variables"] and len(A) == exp["num_constraints"]
    return F, A, B, Cm, w[:ni], w[ni:], exp



@functools.lru_cache(maxsize=2)
def penumbra_libsnark_key(seed: int = 377):
    """A Groth16 key for the reference's Penumbra output circuit on BLS12-377 from the restated arkworks LibSnark generator
    (oracle.groth16.libsnark_setup) with seeded toxic waste -- the reference's own circuit.pk is absent upstream. Returns
    (fixture tuple, key dict, vk dict, ark-serialized ProvingKey bytes, oracle MSM through oracle/c)."""
    import random
    from oracle import arkfmt, cbridge as cb, groth16 as g16
    fx = load_penumbra_fixture()
    F, A, B, Cm, pub, wit, exp = fx
    G1, G2 = cv.BLS377_G1, cv.BLS377_G2
    rng = random.Random(seed)
    toxic = tuple(rng.randrange(1, F.p) for _ in range(5))

    def fixed_base(group, scalars):
        return cv.unpack_points((G1, G2)[group], cb.fixed_base_mul(3, group, fl.pack(F, scalars, mont=False)))

    def msm(G, pts, sc):
        if not pts:
            return None
        return cv.unpack_points(G, cb.msm_fast(3, 0 if G is G1 else 1, cv.pack_points(G, pts), fl.pack(F, sc)))[0]

    key = g16.libsnark_setup(F, exp["generator"], G1, G2, A, B, Cm, len(pub), len(wit), toxic, fixed_base)
    vk = {"alpha_g1": key["alpha_g1"], "beta_g2": key["beta_g2"], "gamma_g2": key["gamma_g2"], "delta_g2": key["delta_g2"], "ic": key["gamma_abc_g1"]}
    return fx, key, vk, arkfmt.ser_groth16_proving_key(key, G1.F.p, 48), msm


# ---- raw limbs of the signed lazy field (field29.hpp FpS): B bits x NL limbs per base field ---------------------------------------
LAZY_LIMBS = {"bn254": (29, 9), "bls12_381": (28, 14), "bls12_377": (28, 14), "grumpkin": (29, 9)}


def fp2_raw_operands(curve, p, r, n):
    """n operand sets (a, b, c, d) of Fp2 elements as raw signed limbs for the Fp2 product tests: limbs 0 .. NL-2 from the five patterns
    all +lim, all -lim, alternating, random sign at lim, random in range (lim = 2^B + 8, the normalised-operand bound), the top limb
    within the value contract |x| < 8p. The first five sets are the pure patterns. -> (list of 4 x (c0 limbs, c1 limbs), flat int32)"""
    B, NL = LAZY_LIMBS[curve]
    lim = (1 << B) + 8
    top = 4 * (p >> (B * (NL - 1)))
    tl = lambda: [r.randrange(-top, top + 1)]
    patterns = [
        lambda: [lim] * (NL - 1) + tl(), lambda: [-lim] * (NL - 1) + tl(), lambda: [lim if i % 2 else -lim for i in range(NL - 1)] + tl(),
        lambda: [r.choice((lim, -lim)) for _ in range(NL - 1)] + tl(), lambda: [r.randrange(-lim, lim + 1) for _ in range(NL - 1)] + tl(),
    ]
    els = []
    for j in range(n):
        if j < 5:
            els.append([(patterns[j](), patterns[j]()) for _ in range(4)])
        else:
            els.append([(patterns[r.randrange(5)](), patterns[r.randrange(5)]()) for _ in range(4)])
    flat = np.array([x for e in els for el in e for comp in el for x in comp], dtype=np.int32)
    return els, flat


def _respell(limbs, B, r, moves):
    """Random borrow moves l[i] -= 2^B, l[i+1] += 1 and the reverse: the same integer, limbs 0 .. NL-2 kept within |l| <= 2^B + 2 (the
    class a difference of two reduction outputs belongs to); the top limb is free."""
    l = list(limbs)
    NL, lim = len(l), (1 << B) + 2
    for _ in range(moves):
        i = r.randrange(NL - 1)
        s = r.choice((1, -1))
        a, b = l[i] - s * (1 << B), l[i + 1] + s
        if abs(a) <= lim and (i + 1 == NL - 1 or abs(b) <= lim):
            l[i], l[i + 1] = a, b
    return l


def _digits(v, B, NL):
    """canonical digits of a (possibly negative) integer: limbs 0 .. NL-2 in [0, 2^B), the signed top limb takes the rest"""
    return [(v >> (B * i)) & ((1 << B) - 1) for i in range(NL - 1)] + [v >> (B * (NL - 1))]


def zero_test_cases(p, B, NL, r, spellings=12):
    """Inputs of the lazy field's zero tests as (limbs, kind):
    'zero'     k p for every k in -7 .. 7, canonical digits and `spellings` random re-spellings each: maybe_zero() and is_zero_slow() true;
    'limb0'    such a spelling +/- 2^B or +/- 2^(2B) (limb 0 unchanged): maybe_zero() true, is_zero_slow() false -- the slow test decides;
    'nonzero'  such a spelling +/- 1, and random values in (-7p, 7p) that are no multiple of p: is_zero() and is_zero_slow() false."""
    lim = (1 << B) + 2
    val = lambda l: sum(x << (B * i) for i, x in enumerate(l))
    cases = []
    for k in range(-7, 8):
        base = _digits(k * p, B, NL)
        sp = [base] + [_respell(base, B, r, 4 * NL) for _ in range(spellings)]
        for l in sp:
            assert val(l) == k * p and all(abs(x) <= lim for x in l[:-1])
            cases.append((l, "zero"))
        for limb, kind in ((1, "limb0"), (2, "limb0"), (0, "nonzero")):
            for sgn in (1, -1):
                for l in sp[1:4]:
                    if abs(l[limb] + sgn) <= lim:
                        m = list(l)
                        m[limb] += sgn
                        cases.append((m, kind))
    for _ in range(8 * spellings):
        v = r.randrange(-7 * p, 7 * p)
        if v % p:
            cases.append((_respell(_digits(v, B, NL), B, r, 4 * NL), "nonzero"))
    return cases


def check_zero_flags(flags, comps, ctx):
    """flags = maybe_zero() | is_zero_slow() << 1 | is_zero() << 2 of an element whose components are `comps` (zero_test_cases entries;
    one for a base-field element, two for Fp2: every predicate is the conjunction over the components)."""
    kinds = [k for _, k in comps]
    zero = all(k == "zero" for k in kinds)
    maybe, slow, both = bool(flags & 1), bool(flags & 2), bool(flags & 4)
    assert slow == zero, ("is_zero_slow()", kinds, ctx)
    assert both == zero, ("is_zero()", kinds, ctx)
    if all(k in ("zero", "limb0") for k in kinds):
        assert maybe, ("maybe_zero() misses a multiple of p in its window (or a value with the same limb 0)", kinds, ctx)


# ---- edge-value case lists of the element-wise kernels (vec_ops.hip), shared by the host self-test and the device tests -------------
def elementwise_edge_set(F):
    """edge_elems(F) reduced mod p, plus (p + 1) / 2 and p - 3."""
    return [v % F.p for v in edge_elems(F)] + [(F.p + 1) // 2, F.p - 3]


def elementwise_cases(F):
    """Operands and expected values (Python integers) of every per-element expression of vec_ops.hip at the edges of the field:
    'pairs'      (a, b): all pairs of the edge set E;
    'mul_sub'    (a, b, c, a b - c): every pair with c cycling through E, and with c = a b - t for t in {0, 1, p - 1} (result exactly t);
    'rep3'       (la, lb, ra, rb, mask, sub, la (ra + rb) + lb ra + mask - sub): every pair (la, ra), (lb, rb, mask, sub) cycling through 13
                 fixed tuples of E, then with the mask solved for a result of exactly 0, 1, p - 1; the same with sub = None (absent); the
                 same with mask = None, where sub is the operand that is solved;
    'to_shamir'  (a, b, x, y, a x + b y): every pair as the share, (x, y) = the three parties' translation points and (0, 0), (1, p - 1),
                 (p - 1, p - 1)."""
    from oracle import mpc
    p = F.p
    E = elementwise_edge_set(F)
    ne = len(E)
    pairs = [(a, b) for a in E for b in E]
    tuples = [(E[(5 * k + 1) % ne], E[(7 * k + 3) % ne], E[(3 * k + 5) % ne], E[(11 * k + 7) % ne]) for k in range(13)]
    targets = (0, 1, p - 1)
    mul_sub, rep3 = [], []
    for k, (a, b) in enumerate(pairs):
        for c in [E[(k + k // ne) % ne]] + [(a * b - t) % p for t in targets]:
            mul_sub.append((a, b, c, (a * b - c) % p))
    for with_mask, with_sub in ((True, True), (True, False), (False, True)):
        for k, (la, ra) in enumerate(pairs):
            lb, rb, m, s = tuples[k % len(tuples)]
            prod = la * (ra + rb) + lb * ra
            s_ = s if with_sub else 0
            variants = [(m if with_mask else None, s if with_sub else None)]
            for t in targets:
                variants.append(((t - prod + s_) % p, s if with_sub else None) if with_mask else (None, (prod - t) % p))
            for mm, ss in variants:
                rep3.append((la, lb, ra, rb, mm, ss, (prod + (mm or 0) - (ss or 0)) % p))
    points = [mpc.rep3_to_shamir_points(F, party) for party in range(3)] + [(0, 0), (1, p - 1), (p - 1, p - 1)]
    to_shamir = [(a, b, x, y, (a * x + b * y) % p) for x, y in points for a, b in pairs]
    return {"pairs": pairs, "mul_sub": mul_sub, "rep3": rep3, "to_shamir": to_shamir}
