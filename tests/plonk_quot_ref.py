"""Round3::compute_t of the circom PLONK prover (co-circom/co-plonk/src/round3.rs:246-502) restated in Python integers, loop by loop as the
reference writes it: the `if mod_i != 0` branches, the in-place division by Z_H and the order of the additions are kept, so that this file
is a statement of its own and not a copy of the closed forms in include/cosnarks_hip.h. A share is a tuple of `ncomp` integers; `Ops` is
the reference's CircomPlonkProver for one party (plain / Shamir: one component, Rep3: {a, b})."""


class Ops:
    """mpc-core/src/protocols/rep3/arithmetic.rs and shamir/arithmetic.rs, the linear operations compute_t uses."""

    def __init__(self, p, protocol, party):
        self.p, self.protocol, self.party, self.ncomp = p, protocol, party, protocol + 1

    def default(self):
        return (0,) * self.ncomp

    def add(self, a, b):
        return tuple((x + y) % self.p for x, y in zip(a, b))

    def sub(self, a, b):
        return tuple((x - y) % self.p for x, y in zip(a, b))

    def mul_with_public(self, a, c):
        return tuple(x * c % self.p for x in a)

    def add_mul_public(self, a, b, c):
        return self.add(a, self.mul_with_public(b, c))

    def add_with_public(self, a, c):
        """rep3/arithmetic.rs:41-49: party 0 adds to a, party 1 to b, party 2 nothing; shamir/arithmetic.rs:45 and plain: the one component."""
        if self.protocol == 0:
            return ((a[0] + c) % self.p,)
        if self.party == 0:
            return ((a[0] + c) % self.p, a[1])
        if self.party == 1:
            return (a[0], (a[1] + c) % self.p)
        return a

    def neg(self, a):
        return tuple(-x % self.p for x in a)


def get_z1(p, root_of_unity):
    zero = 0
    neg_1 = (zero - 1) % p
    neg_2 = (neg_1 - 1) % p
    return [zero, (neg_1 + root_of_unity) % p, neg_2, (neg_1 - root_of_unity) % p]


def get_z2(p, root_of_unity):
    zero = 0
    two = 2
    four = two * two % p
    neg_2 = (zero - two) % p
    neg2_root_unity = neg_2 * root_of_unity % p
    return [zero, neg2_root_unity, four, (0 - neg2_root_unity) % p]


def get_z3(p, root_of_unity):
    zero = 0
    two = 2
    neg_eight = -(two * two % p * two) % p
    two_root_unity = two * root_of_unity % p
    return [zero, (two + two_root_unity) % p, neg_eight, (two - two_root_unity) % p]


def first_w_product(T, length, b, pow_plus2_root_of_unity):
    """round3.rs:269-274 -> ap, bp, cp"""
    p = T.p
    w = 1
    ap, bp, cp = [], [], []
    for _ in range(length):
        ap.append(T.add_mul_public(b[1], b[0], w))
        bp.append(T.add_mul_public(b[3], b[2], w))
        cp.append(T.add_mul_public(b[5], b[4], w))
        w = w * pow_plus2_root_of_unity % p
    return ap, bp, cp


def second_w_product(T, length, z1, pow_root_of_unity, pow_plus2_root_of_unity, polys, zkey, b, prods, beta, gamma, k1, k2):
    """round3.rs:320-419. polys: a, b, c, z, buffer_a; zkey: qm, ql, qr, qo, qc, s1, s2, s3 (evaluations) and lagrange (a list of them);
    prods: a_b, a_bp, ap_b, ap_bp, ap, bp, cp. -> dict of e1, e1z, e2a..e2d, zp, e3a..e3d, zwp, pi"""
    p = T.p
    o = {k: [] for k in ("pi", "e1", "e1z", "e2a", "e2b", "e2c", "e2d", "zp", "e3a", "e3b", "e3c", "e3d", "zwp")}
    w = 1
    for i in range(length):
        a = polys["a"][i]
        b_ = polys["b"][i]
        c = polys["c"][i]
        z = polys["z"][i]
        qm = zkey["qm"][i]
        ql = zkey["ql"][i]
        qr = zkey["qr"][i]
        qo = zkey["qo"][i]
        qc = zkey["qc"][i]
        s1 = zkey["s1"][i]
        s2 = zkey["s2"][i]
        s3 = zkey["s3"][i]
        a_bp = prods["a_bp"][i]
        a_b = prods["a_b"][i]
        ap_b = prods["ap_b"][i]
        ap = prods["ap"][i]
        bp = prods["bp"][i]

        w2 = w * w % p
        zp_lhs = T.mul_with_public(b[6], w2)
        zp_rhs = T.mul_with_public(b[7], w)
        zp_ = T.add(zp_lhs, zp_rhs)
        zp_ = T.add(b[8], zp_)
        o["zp"].append(zp_)

        w_w = w * pow_root_of_unity % p
        w_w2 = w_w * w_w % p
        zw = polys["z"][(length + 4 + i) % length]
        zwp_lhs = T.mul_with_public(b[6], w_w2)
        zwp_rhs = T.mul_with_public(b[7], w_w)
        zwp_ = T.add(zwp_lhs, zwp_rhs)
        zwp_ = T.add(b[8], zwp_)
        o["zwp"].append(zwp_)

        a0 = T.add(a_bp, ap_b)
        mod_i = i % 4
        if mod_i != 0:
            z1_ = z1[mod_i]
            ap_bp = prods["ap_bp"][i]
            tmp = T.mul_with_public(ap_bp, z1_)
            a0 = T.add(a0, tmp)

        e1_, e1z_ = a_b, a0
        e1_ = T.mul_with_public(e1_, qm)
        e1z_ = T.mul_with_public(e1z_, qm)

        e1_ = T.add_mul_public(e1_, a, ql)
        e1z_ = T.add_mul_public(e1z_, ap, ql)

        e1_ = T.add_mul_public(e1_, b_, qr)
        e1z_ = T.add_mul_public(e1z_, bp, qr)

        e1_ = T.add_mul_public(e1_, c, qo)
        e1z_ = T.add_mul_public(e1z_, prods["cp"][i], qo)

        pi = T.default()
        for j, lagrange in enumerate(zkey["lagrange"]):
            tmp = T.mul_with_public(polys["buffer_a"][j], lagrange[i])
            pi = T.sub(pi, tmp)
        o["pi"].append(pi)

        e1_ = T.add(e1_, pi)
        e1_ = T.add_with_public(e1_, qc)
        o["e1"].append(e1_)
        o["e1z"].append(e1z_)

        betaw = beta * w % p
        o["e2a"].append(T.add_with_public(a, (betaw + gamma) % p))
        o["e2b"].append(T.add_with_public(b_, (betaw * k1 + gamma) % p))
        o["e2c"].append(T.add_with_public(c, (betaw * k2 + gamma) % p))
        o["e2d"].append(z)
        o["e3a"].append(T.add_with_public(a, (s1 * beta + gamma) % p))
        o["e3b"].append(T.add_with_public(b_, (s2 * beta + gamma) % p))
        o["e3c"].append(T.add_with_public(c, (s3 * beta + gamma) % p))
        o["e3d"].append(zw)
        w = w * pow_plus2_root_of_unity % p
    return o


def mul4vec_post(T, a, b, c, d, i, z1, z2, z3):
    """round3.rs:88-105"""
    mod_i = i % 4
    rz = a[i]
    if mod_i != 0:
        tmp = T.mul_with_public(b[i], z1[mod_i])
        rz = T.add(tmp, rz)
        tmp = T.mul_with_public(c[i], z2[mod_i])
        rz = T.add(rz, tmp)
        tmp = T.mul_with_public(d[i], z3[mod_i])
        rz = T.add(rz, tmp)
    return rz


def t_tz(T, length, z1, z2, z3, e1, e1z, z, zp, e2, e2z, e3, e3z, lagrange0, alpha, alpha2):
    """round3.rs:435-467. e2z, e3z: lists of the four vectors X_0..X_3. -> t_vec, tz_vec"""
    p = T.p
    t_vec, tz_vec = [], []
    for i in range(length):
        e2_ = e2[i]
        e2z_ = mul4vec_post(T, e2z[0], e2z[1], e2z[2], e2z[3], i, z1, z2, z3)
        e3_ = e3[i]
        e3z_ = mul4vec_post(T, e3z[0], e3z[1], e3z[2], e3z[3], i, z1, z2, z3)

        z_ = z[i]
        zp_ = zp[i]

        e2_ = T.mul_with_public(e2_, alpha)
        e2z_ = T.mul_with_public(e2z_, alpha)

        e3_ = T.mul_with_public(e3_, alpha)
        e3z_ = T.mul_with_public(e3z_, alpha)

        e4 = T.add_with_public(z_, -1 % p)
        e4 = T.mul_with_public(e4, lagrange0[i])
        e4 = T.mul_with_public(e4, alpha2)

        e4z = T.mul_with_public(zp_, lagrange0[i])
        e4z = T.mul_with_public(e4z, alpha2)

        t = T.add(e1[i], e2_)
        t = T.sub(t, e3_)
        t = T.add(t, e4)

        tz = T.add(e1z[i], e2z_)
        tz = T.sub(tz, e3z_)
        tz = T.add(tz, e4z)

        t_vec.append(t)
        tz_vec.append(tz)
    return t_vec, tz_vec


def divide_by_zh_in_place(T, coefficients_t, domain_size):
    """round3.rs:469-478, in place: the loop reads the chunk below, which it has already updated. Returns the same list."""
    length = len(coefficients_t)
    for i in range(domain_size):
        coefficients_t[i] = T.neg(coefficients_t[i])
    for i in range(domain_size, length):
        a_lhs = coefficients_t[i - domain_size]
        a_rhs = coefficients_t[i]
        coefficients_t[i] = T.sub(a_lhs, a_rhs)
    return coefficients_t


def finish(T, domain_size, coefficients_t, coefficients_tz, b9, b10):
    """round3.rs:468-498 after the two iffts -> t1, t2, t3, and the whole t_final (the coefficients the split drops included)"""
    coefficients_t = divide_by_zh_in_place(T, list(coefficients_t), domain_size)
    t_final = [T.add(lhs, rhs) for lhs, rhs in zip(coefficients_t, coefficients_tz)]
    it = iter(t_final)
    t1, t2 = [], []
    for _ in range(domain_size):
        t1.append(next(it))
    for _ in range(domain_size):
        t2.append(next(it))
    t3 = [next(it) for _ in range(domain_size + 6)]
    t1.append(b9)

    t2[0] = T.sub(t2[0], b9)
    t2.append(b10)

    t3[0] = T.sub(t3[0], b10)
    return t1, t2, t3, t_final


def mul_vec_plain(T, a, b):
    """PlainPlonkDriver::mul_vec: the product of the single components"""
    assert T.protocol == 0
    return [(x[0] * y[0] % T.p,) for x, y in zip(a, b)]


def mul4vec_plain(T, a, b, c, d, ap, bp, cp, dp):
    """round3.rs:20-86 with the plain driver's mul_vec / add_mul_vec -> [r, a0, a1, a2, a3]"""
    m = lambda x, y: mul_vec_plain(T, x, y)
    am = lambda acc, x, y: [T.add(s, t) for s, t in zip(acc, m(x, y))]
    a_b, a_bp, ap_b, ap_bp = m(a, b), m(a, bp), m(ap, b), m(ap, bp)
    c_d, c_dp, cp_d, cp_dp = m(c, d), m(c, dp), m(cp, d), m(cp, dp)
    r = m(a_b, c_d)
    a0 = m(ap_b, c_d)
    a0 = am(a0, a_bp, c_d)
    a0 = am(a0, a_b, cp_d)
    a0 = am(a0, a_b, c_dp)
    a1 = m(ap_bp, c_d)
    a1 = am(a1, ap_b, cp_d)
    a1 = am(a1, ap_b, c_dp)
    a1 = am(a1, a_bp, cp_d)
    a1 = am(a1, a_bp, c_dp)
    a1 = am(a1, a_b, cp_dp)
    a2 = m(a_bp, cp_dp)
    a2 = am(a2, ap_b, cp_dp)
    a2 = am(a2, ap_bp, c_dp)
    a2 = am(a2, ap_bp, cp_d)
    a3 = m(ap_bp, cp_dp)
    return [r, a0, a1, a2, a3]


def compute_t_plain(p, n, w_ext, polys, zkey, b, beta, gamma, alpha, k1, k2, ifft):
    """Round3::compute_t for the plain driver. w_ext: the generator of the extended domain (4 n points); ifft: list of ints -> list of ints
    on that domain. -> t1, t2, t3 (lists of 1-tuples)"""
    T = Ops(p, 0, 0)
    length = 4 * n
    root2 = pow(w_ext, n, p)
    z1, z2, z3 = get_z1(p, root2), get_z2(p, root2), get_z3(p, root2)
    pow_root = pow(w_ext, 4, p)
    ap, bp, cp = first_w_product(T, length, b, w_ext)
    prods = {"a_b": mul_vec_plain(T, polys["a"], polys["b"]), "a_bp": mul_vec_plain(T, polys["a"], bp),
             "ap_b": mul_vec_plain(T, polys["b"], ap), "ap_bp": mul_vec_plain(T, ap, bp), "ap": ap, "bp": bp, "cp": cp}
    o = second_w_product(T, length, z1, pow_root, w_ext, polys, zkey, b, prods, beta, gamma, k1, k2)
    e2, *e2z = mul4vec_plain(T, o["e2a"], o["e2b"], o["e2c"], o["e2d"], ap, bp, cp, o["zp"])
    e3, *e3z = mul4vec_plain(T, o["e3a"], o["e3b"], o["e3c"], o["e3d"], ap, bp, cp, o["zwp"])
    t_vec, tz_vec = t_tz(T, length, z1, z2, z3, o["e1"], o["e1z"], polys["z"], o["zp"], e2, e2z, e3, e3z, zkey["lagrange"][0], alpha, alpha * alpha % p)
    ct = [(x,) for x in ifft([t[0] for t in t_vec])]
    ctz = [(x,) for x in ifft([t[0] for t in tz_vec])]
    t1, t2, t3, _ = finish(T, n, ct, ctz, b[9], b[10])
    return t1, t2, t3


# ---- inputs for the tests of the four stages, and what the loops above make of them ---------------------------------------------------
SHARE_NAMES = ["a", "b", "c", "z", "a_b", "a_bp", "ap_b", "ap_bp", "ap", "bp", "cp"]          # stage (b), the ABI's order
PUBLIC_NAMES = ["qm", "ql", "qr", "qo", "qc", "s1", "s2", "s3"]
OPERAND_OUTS = ["pi", "e1", "e1z", "e2a", "e2b", "e2c", "e3a", "e3b", "e3c", "e3d"]
COMBINE_NAMES = ["e1", "e1z", "z", "zp", "e2", "e2z_0", "e2z_1", "e2z_2", "e2z_3", "e3", "e3z_0", "e3z_1", "e3z_2", "e3z_3"]  # stage (c)


def flat(vec):
    """a list of shares -> the integers in memory order (component-interleaved)"""
    return [x for s in vec for x in s]


def stage_case(p, protocol, party, n, w_ext, n_public, draw, zkey=None, k12=None):
    """Inputs of the four stages and the restatement's outputs. Every share vector of a stage is drawn independently (a stage is tested as
    a function of its inputs, not of the stage before). draw(): one field element; zkey: real public vectors (qm .. s3, lagrange) or None
    for drawn ones; k12: the zkey's (k1, k2) or None."""
    T = Ops(p, protocol, party)
    N = 4 * n
    sh = lambda: tuple(draw() for _ in range(T.ncomp))
    vec = lambda: [sh() for _ in range(N)]
    pub = lambda: [draw() for _ in range(N)]
    c = {"T": T, "N": N, "n": n}
    c["b"] = [sh() for _ in range(11)]
    c["shares"] = {k: vec() for k in SHARE_NAMES}
    if zkey is None:
        zkey = {k: pub() for k in PUBLIC_NAMES}
        zkey["lagrange"] = [pub() for _ in range(max(n_public, 1))]
    c["zkey"] = dict(zkey)
    c["lagrange1"] = zkey["lagrange"][0]
    c["zkey"]["lagrange"] = zkey["lagrange"][:n_public]
    c["buffer_a"] = [sh() for _ in range(n_public)]
    c["beta"], c["gamma"], c["alpha"], c["k1"], c["k2"] = draw(), draw(), draw(), draw(), draw()
    if k12 is not None:
        c["k1"], c["k2"] = k12
    c["combine"] = {k: vec() for k in COMBINE_NAMES}
    c["ct"], c["ctz"] = vec(), vec()

    root2 = pow(w_ext, n, p)
    z1, z2, z3 = get_z1(p, root2), get_z2(p, root2), get_z3(p, root2)
    c["z123"] = z1 + z2 + z3
    ap, bp, cp = first_w_product(T, N, c["b"], w_ext)
    polys = {k: c["shares"][k] for k in ("a", "b", "c", "z")}
    polys["buffer_a"] = c["buffer_a"]
    o = second_w_product(T, N, z1, pow(w_ext, 4, p), w_ext, polys, c["zkey"], c["b"], c["shares"], c["beta"], c["gamma"], c["k1"], c["k2"])
    c["want_blinders"] = [ap, bp, cp, o["zp"], o["zwp"]]
    c["want_operands"] = [o[k] for k in OPERAND_OUTS]
    m = c["combine"]
    t_vec, tz_vec = t_tz(T, N, z1, z2, z3, m["e1"], m["e1z"], m["z"], m["zp"], m["e2"], [m["e2z_%d" % k] for k in range(4)], m["e3"],
                         [m["e3z_%d" % k] for k in range(4)], c["lagrange1"], c["alpha"], c["alpha"] * c["alpha"] % p)
    c["want_combine"] = [t_vec, tz_vec]
    t1, t2, t3, _ = finish(T, n, c["ct"], c["ctz"], c["b"][9], c["b"][10])
    c["want_finish"] = [t1, t2, t3]
    return c


def poly_times_zh(p, q, n):
    """q(X) (X^n - 1), all len(q) + n coefficients"""
    out = [0] * (len(q) + n)
    for i, x in enumerate(q):
        out[i] = (out[i] - x) % p
        out[i + n] = (out[i + n] + x) % p
    return out


def division_case(p, T, n, r, with_rest):
    """q of 3 n + 6 coefficients and ct = the low 4 n coefficients of q (X^n - 1) -> (q, ct, ctz, b9, b10) as lists of shares"""
    comps = []
    for _ in range(T.ncomp):
        q = [r.randrange(p) for _ in range(3 * n + 6)]
        comps.append((q, poly_times_zh(p, q, n)[:4 * n]))
    q = [tuple(c[0][i] for c in comps) for i in range(3 * n + 6)]
    ct = [tuple(c[1][i] for c in comps) for i in range(4 * n)]
    sh = (lambda: tuple(r.randrange(p) for _ in range(T.ncomp))) if with_rest else T.default
    return q, ct, [sh() for _ in range(4 * n)], sh(), sh()


def check_division(T, n, q, ct, ctz, b9, b10, t1, t2, t3):
    """what the finish must return for division_case's inputs, stated from q itself, and the restatement's word on the dropped coefficients"""
    tf = [T.add(x, y) for x, y in zip(q + [T.default()] * (n - 6), ctz)]
    want_t1, want_t2, want_t3, t_final = finish(T, n, ct, ctz, b9, b10)
    assert t_final == tf                                  # the recurrence inverts the multiplication, and leaves zeros (+ ctz) above 3 n + 6
    assert t1 == tf[:n] + [b9] == want_t1
    assert t2 == [T.sub(tf[n], b9)] + tf[n + 1:2 * n] + [b10] == want_t2
    assert t3 == [T.sub(tf[2 * n], b10)] + tf[2 * n + 1:3 * n + 6] == want_t3
