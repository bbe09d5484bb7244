"""Rounds 2 and 5 of the circom PLONK prover between their network rounds, restated in Python integers from the formulas of the paper
(eprint 2019/953, rounds 2 and 5) and of include/cosnarks_hip.h: the operands of compute_z, rotate_right, blind_coefficients and the ragged
linear combination that is compute_r + compute_wxi. Shares are tuples of `ncomp` integers on the `Ops` class of tests/plonk_quot_ref.py.
Also: a reader for the additions and the A / B / C map sections of a snarkjs PLONK zkey, and a plain prover chain, rounds 1-5, that takes
its challenges and blinders as arguments (no transcript, no commitments). Last, what the CPU and the GPU tests share: one case of the four
entries (entries_case) and the chain on the reference's multiplier2 circuit with fixed challenges (fixture_chain)."""
import functools
import os
import struct

from tests.plonk_quot_ref import Ops, compute_t_plain, flat  # noqa: F401


# ---- the four entries ----------------------------------------------------------------------------------------------------------------
def z_operands(T, n, w, a, b, c, s1, s2, s3, beta, gamma, k1, k2):
    """a, b, c: n shares; s1, s2, s3: the 4 n evaluations on the extended domain, read at 4 i; w: the generator of the n-point domain.
    -> [n1, n2, n3, d1, d2, d3]"""
    p = T.p
    out = [[] for _ in range(6)]
    wi = 1
    for i in range(n):
        out[0].append(T.add_with_public(a[i], (beta * wi + gamma) % p))
        out[1].append(T.add_with_public(b[i], (beta * k1 * wi + gamma) % p))
        out[2].append(T.add_with_public(c[i], (beta * k2 * wi + gamma) % p))
        out[3].append(T.add_with_public(a[i], (beta * s1[4 * i] + gamma) % p))
        out[4].append(T.add_with_public(b[i], (beta * s2[4 * i] + gamma) % p))
        out[5].append(T.add_with_public(c[i], (beta * s3[4 * i] + gamma) % p))
        wi = wi * w % p
    return out


def rotate_right(v, k):
    """out[(i + k) mod n] = v[i]"""
    n = len(v)
    out = [None] * n
    for i in range(n):
        out[(i + k) % n] = v[i]
    return out


def blind_coefficients(T, poly, coeff_rev):
    """poly (n shares) -> n + k shares: poly[j] -= coeff_rev[k - 1 - j], poly[n + j] = coeff_rev[k - 1 - j]"""
    k = len(coeff_rev)
    out = list(poly)
    for j in range(k):
        out[j] = T.sub(out[j], coeff_rev[k - 1 - j])
    return out + [coeff_rev[k - 1 - j] for j in range(k)]


def poly_lincomb(T, shares, share_coeffs, publics, public_coeffs, const0, out_len):
    """out[i] = sum_j cs_j S_j[i] (+) (sum_j cp_j P_j[i] + [i = 0] const0), every vector read as far as it goes"""
    p = T.p
    out = []
    for i in range(out_len):
        acc = T.default()
        for s, c in zip(shares, share_coeffs):
            if i < len(s):
                acc = T.add(acc, T.mul_with_public(s[i], c))
        pub = sum(c * v[i] for v, c in zip(publics, public_coeffs) if i < len(v))
        if i == 0 and const0 is not None:
            pub += const0
        out.append(T.add_with_public(acc, pub % p))
    return out


def div_linear(T, coeffs, root):
    """division by (X - root) from the low coefficients up -> (quotient of len - 1 shares, remainder share)"""
    p = T.p
    inv = pow(root, -1, p)
    out, prev = [], T.default()
    for x in coeffs:
        prev = T.mul_with_public(T.sub(x, prev), -inv % p)
        out.append(prev)
    return out[:-1], out[-1]


def eval_poly(T, coeffs, x):
    acc = T.default()
    for c in reversed(coeffs):
        acc = T.add(T.mul_with_public(acc, x), c)
    return acc


# ---- round 5: the public coefficients of the one linear combination --------------------------------------------------------------------
def lagrange_evaluations(p, n, w, n_public, xi):
    """L_1(xi) .. L_max(1, n_public)(xi) and xi^n"""
    xin = pow(xi, n, p)
    zh = (xin - 1) % p
    ls, wi = [], 1
    for _ in range(max(1, n_public)):
        ls.append(wi * zh % p * pow(n * (xi - wi) % p, -1, p) % p)
        wi = wi * w % p
    return ls, xin


def round5_coefficients(p, n, w, public_inputs, ev, beta, gamma, alpha, xi, v, k1, k2):
    """ev: the round-4 evaluations a, b, c, s1, s2, zw. -> (share coefficients for z, t1, t2, t3, a, b, c; public coefficients for qm, ql, qr,
    qo, qc, s3, s1, s2; const0)"""
    ls, xin = lagrange_evaluations(p, n, w, len(public_inputs), xi)
    zh = (xin - 1) % p
    pi = -sum(l * x for l, x in zip(ls, public_inputs)) % p
    ea, eb, ec, es1, es2, ezw = (ev[k] for k in ("a", "b", "c", "s1", "s2", "zw"))
    betaxi = beta * xi % p
    e2 = (ea + betaxi + gamma) * (eb + betaxi * k1 + gamma) % p * (ec + betaxi * k2 + gamma) % p * alpha % p
    e3 = (ea + beta * es1 + gamma) * (eb + beta * es2 + gamma) % p * ezw % p * alpha % p
    e4 = alpha * alpha % p * ls[0] % p
    r0 = (pi - e3 * (ec + gamma) - e4) % p
    cs = [(e2 + e4) % p, -zh % p, -zh * xin % p, -zh * xin % p * xin % p, v[0], v[1], v[2]]
    cp = [ea * eb % p, ea, eb, ec, 1, -e3 * beta % p, v[3], v[4]]
    const0 = (r0 - v[0] * ea - v[1] * eb - v[2] * ec - v[3] * es1 - v[4] * es2) % p
    return cs, cp, const0


# ---- the zkey sections the wire buffers need (snarkjs PLONK zkey: 3 = additions, 4 / 5 / 6 = the A / B / C maps) -----------------------
SECTION_ADDITIONS, SECTION_A_MAP, SECTION_B_MAP, SECTION_C_MAP = 3, 4, 5, 6


def read_additions_and_maps(data, zk):
    """data: the zkey's bytes, zk: oracle.zkey.parse_plonk_zkey(data) -> (additions [(signal1, signal2, factor1, factor2)], map_a, map_b, map_c)"""
    from oracle.zkey import _sections
    secs = _sections(data, b"zkey")
    F, n8r = zk.Fr, zk.n8r
    off, ln = secs[SECTION_ADDITIONS][0]
    assert ln == zk.n_additions * (8 + 2 * n8r)
    additions = []
    for _ in range(zk.n_additions):
        s1, s2 = struct.unpack_from("<II", data, off)
        f1 = F.from_mont(int.from_bytes(data[off + 8:off + 8 + n8r], "little"))
        f2 = F.from_mont(int.from_bytes(data[off + 8 + n8r:off + 8 + 2 * n8r], "little"))
        additions.append((s1, s2, f1, f2))
        off += 8 + 2 * n8r
    maps = []
    for sec in (SECTION_A_MAP, SECTION_B_MAP, SECTION_C_MAP):
        off, ln = secs[sec][0]
        assert ln == 4 * zk.n_constraints
        maps.append(list(struct.unpack_from("<%dI" % zk.n_constraints, data, off)))
    return additions, maps[0], maps[1], maps[2]


def wire_buffers(p, zk, additions, maps, witness):
    """round 1 before the transforms: the addition witnesses and buffer_a, buffer_b, buffer_c (n values each). witness: the .wtns values;
    index 0 (the constant one) counts as zero, as the reference's PlonkWitness::new has it."""
    w = list(witness)
    w[0] = 0
    n_plain = zk.n_vars - zk.n_additions
    assert len(w) == n_plain
    for s1, s2, f1, f2 in additions:
        w.append((w[s1] * f1 + w[s2] * f2) % p)
    return [[w[i] for i in m] + [0] * (zk.domain_size - len(m)) for m in maps]


def prove_chain_plain(F, zk, additions, maps, witness, b, beta, gamma, alpha, xi, v):
    """Rounds 1-5 of the plain prover without transcript and commitments. b: the 11 blinders (integers). -> dict of every vector a device
    chain has to reproduce (lists of integers)"""
    from oracle import ntt
    p, n = F.p, zk.domain_size
    T = Ops(p, 0, 0)
    dom, ext = ntt.Domain.snarkjs(F, n), ntt.Domain.snarkjs(F, 4 * n)
    w = dom.gen
    assert pow(ext.gen, 4, p) == w
    sh = lambda vec: [(x,) for x in vec]
    un = lambda vec: [x[0] for x in vec]
    o = {}
    # round 1
    buffers = wire_buffers(p, zk, additions, maps, witness)
    poly, evals = {}, {}
    for name, buf, j in zip("abc", buffers, (0, 2, 4)):
        co = dom.ifft(buf)
        evals[name] = ext.fft(co)
        poly[name] = un(blind_coefficients(T, sh(co), sh(b[j:j + 2])))
    # round 2
    S = {k: zk.polys[k] for k in ("S1", "S2", "S3")}
    ops = z_operands(T, n, w, sh(buffers[0]), sh(buffers[1]), sh(buffers[2]), S["S1"][1], S["S2"][1], S["S3"][1], beta, gamma, zk.k1, zk.k2)
    o["operands"] = [un(x) for x in ops]
    num, den, acc_n, acc_d = [], [], 1, 1
    for i in range(n):
        acc_n = acc_n * ops[0][i][0] * ops[1][i][0] * ops[2][i][0] % p
        acc_d = acc_d * ops[3][i][0] * ops[4][i][0] * ops[5][i][0] % p
        num.append(acc_n)
        den.append(pow(acc_d, -1, p))
    buffer_z = rotate_right([x * y % p for x, y in zip(num, den)], 1)
    o["buffer_z"] = buffer_z
    co = dom.ifft(buffer_z)
    evals["z"] = ext.fft(co)
    poly["z"] = un(blind_coefficients(T, sh(co), sh(b[6:9])))
    # round 3
    zkey = {k.lower(): zk.polys[k][1] for k in ("Qm", "Ql", "Qr", "Qo", "Qc", "S1", "S2", "S3")}
    zkey["lagrange"] = [l[1] for l in zk.lagrange]
    polys = {k: sh(evals[k]) for k in "abcz"}
    polys["buffer_a"] = sh(buffers[0][:len(zk.lagrange)])
    t1, t2, t3 = compute_t_plain(p, n, ext.gen, polys, zkey, sh(b), beta, gamma, alpha, zk.k1, zk.k2, ext.ifft)
    poly["t1"], poly["t2"], poly["t3"] = un(t1), un(t2), un(t3)
    o["poly"] = poly
    # round 4
    xiw = xi * w % p
    ev = {"a": ntt.eval_poly_at(F, poly["a"], xi), "b": ntt.eval_poly_at(F, poly["b"], xi), "c": ntt.eval_poly_at(F, poly["c"], xi),
          "s1": ntt.eval_poly_at(F, S["S1"][0], xi), "s2": ntt.eval_poly_at(F, S["S2"][0], xi), "zw": ntt.eval_poly_at(F, poly["z"], xiw)}
    o["evals"] = ev
    # round 5
    public_inputs = list(witness[1:zk.n_public + 1])
    cs, cp, const0 = round5_coefficients(p, n, w, public_inputs, ev, beta, gamma, alpha, xi, v, zk.k1, zk.k2)
    o["coefficients"] = (cs, cp, const0)
    shares = [sh(poly[k]) for k in ("z", "t1", "t2", "t3", "a", "b", "c")]
    publics = [zk.polys[k][0] for k in ("Qm", "Ql", "Qr", "Qo", "Qc", "S3", "S1", "S2")]
    o["wxi_num"] = un(poly_lincomb(T, shares, cs, publics, cp, const0, n + 6))
    q, rem = div_linear(T, sh(o["wxi_num"]), xi)
    o["wxi"], o["wxi_rem"] = un(q), rem[0]
    num = list(poly["z"])
    num[0] = (num[0] - ev["zw"]) % p
    q, rem = div_linear(T, sh(num), xiw)
    o["wxiw"], o["wxiw_rem"] = un(q), rem[0]
    return o


# ---- what the CPU and the GPU tests share: one case of the four entries, and the chain on the reference's own circuit -----------------------
def ext_generator(F, n):
    """a generator of the 4 n-point domain"""
    from oracle import ntt
    return ntt.roots_of_unity(F)[1][(4 * n).bit_length() - 1]


def entries_case(p, T, n, draw, w):
    """inputs of the four entries in the shapes of rounds 2 and 5 and what the restatement makes of them; draw(): one field element"""
    sh = lambda: tuple(draw() for _ in range(T.ncomp))
    vec = lambda k: [sh() for _ in range(k)]
    pub = lambda k: [draw() for _ in range(k)]
    c = {"n": n, "a": vec(n), "b": vec(n), "c": vec(n), "sigma": [pub(4 * n) for _ in range(3)], "ch": [draw() for _ in range(4)]}
    c["want_z"] = z_operands(T, n, w, c["a"], c["b"], c["c"], *c["sigma"], *c["ch"])
    c["blind"] = [vec(k) for k in (1, 2, 3)]
    c["want_blind"] = [blind_coefficients(T, c["a"], cr) for cr in c["blind"]]
    # round 5: z (n + 3), t1, t2 (n + 1), t3 (n + 6), a, b, c (n + 2); qm .. s2 (n)
    c["shares"] = [vec(n + 3), vec(n + 1), vec(n + 1), vec(n + 6), vec(n + 2), vec(n + 2), vec(n + 2)]
    c["cs"] = pub(7)
    c["publics"] = [pub(n) for _ in range(8)]
    c["cp"] = pub(4) + [1] + pub(3)
    c["const0"] = draw()
    c["want_lc"] = poly_lincomb(T, c["shares"], c["cs"], c["publics"], c["cp"], c["const0"], n + 6)
    return c


@functools.lru_cache(maxsize=None)
def fixture_chain(curve):
    """the restated plain chain on tests/golden/Plonk/<curve>/multiplier2 with fixed non-trivial challenges and blinders"""
    from oracle import zkey as Z
    from tests import helpers as H
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "Plonk", curve, "multiplier2")
    data = open(os.path.join(d, "circuit.zkey"), "rb").read()
    zk = Z.parse_plonk_zkey(data)
    witness = Z.parse_wtns(open(os.path.join(d, "witness.wtns"), "rb").read())
    additions, ma, mb, mc = read_additions_and_maps(data, zk)
    F = H.FR[curve]
    r = H.rng(20251)
    b = [r.randrange(1, F.p) for _ in range(11)]
    beta, gamma, alpha, xi = (r.randrange(2, F.p) for _ in range(4))
    v = [r.randrange(2, F.p) for _ in range(5)]
    o = prove_chain_plain(F, zk, additions, (ma, mb, mc), witness, b, beta, gamma, alpha, xi, v)
    o.update(zk=zk, b=b, beta=beta, gamma=gamma, alpha=alpha, xi=xi, v=v, maps=(ma, mb, mc), additions=additions, witness=witness)
    return o
