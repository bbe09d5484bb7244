"""The sumcheck round of co-noir's collaborative UltraHonk prover for the arithmetic, permutation, delta-range and log-derivative lookup
relations, restated in Python integers from co-noir/co-ultrahonk/src/co_decider/: the batch of extend_edges + fold_and_filter +
add_entities (co_sumcheck/co_sumcheck_round.rs:54-73, types_batch.rs:105-130, relations/mod.rs:69-80), the `accumulate` bodies of
relations/ultra_arithmetic_relation.rs:88-239, permutation_relation.rs:70-150 and :202-249, delta_range_constraint_relation.rs:126-216 and
logderiv_lookup_relation.rs:77-168 and :255-312 cut at their mul_many calls, fold_accumulator! (relations/mod.rs:45-57) and the reshare of
arith.r0 (:140-162). Written in the reference's shape -- whole batch vectors, one vector operation after another -- where the device
evaluates one element at a time, so that the two can be compared.

A share vector is a flat list of ints with `ncomp` values per element: one for protocol 0 (plain and Shamir), {a, b} for Rep3 (protocol 1).
Also here, for the tests only: in-process networks for one plain party, three Rep3 parties and three Shamir parties of degree 1 (whose
degree reduction is open-and-reshare), and the driver that makes the reference's call sequence over a set of stage functions."""
from tests import honk_relations_ref as R

POINTS = 7
SHARED = R.WITNESS + R.SHIFTED
STAGE_ACC = {"arith_r0": [6], "arith_r1": [5], "perm": [6, 3], "delta": [6, 6, 6, 6], "lookup_r0": [5], "lookup": [5, 3]}


def pub_comp(protocol, party):
    """the component that takes a public addend: a for protocol 0 and Rep3 party 0, b for Rep3 party 1, none for Rep3 party 2"""
    return 0 if protocol == 0 else {0: 0, 1: 1, 2: None}[party]


def select_edges(polys, col, edge_begin, edge_end):
    """can_skip of ultra_arithmetic_relation.rs:247-249 / delta_range_constraint_relation.rs:94-96 -> the kept e >> 1, ascending"""
    return [e >> 1 for e in range(edge_begin, edge_end, 2) if polys[col][e] or polys[col][e + 1]]


class View:
    """What one party sees of one relation's batch: polys[c] is a flat list (ncomp values per element for the 13 shared columns)."""

    def __init__(self, p, polys, protocol, party, params, edge_begin, edge_end, edge_list=None, scaling=None, stride=1):
        self.p, self.polys, self.protocol, self.party, self.params = p, polys, protocol, party, params
        self.ncomp, self.pc = protocol + 1, pub_comp(protocol, party)
        self.edge_begin, self.edge_end, self.edge_list, self.scaling, self.stride = edge_begin, edge_end, edge_list, scaling, stride
        self.edges = [2 * i for i in edge_list] if edge_list is not None else list(range(edge_begin, edge_end, 2))
        self.m = len(self.edges)

    def _ext(self, v0, v1):
        return [(v0 + k * (v1 - v0)) % self.p for k in range(POINTS)]

    def pub(self, c):
        """the batch of a public column: 7 m ints"""
        v = self.polys[c]
        return [x for e in self.edges for x in self._ext(v[e], v[e + 1])]

    def sh(self, c):
        """the batch of a shared column: 7 m tuples of ncomp ints"""
        v, nc = self.polys[c], self.ncomp
        out = []
        for e in self.edges:
            comps = [self._ext(v[e * nc + cc], v[(e + 1) * nc + cc]) for cc in range(nc)]
            out += list(zip(*comps))
        return out

    def sf(self):
        """scaling_factors of Relation::add_edge: each edge's factor seven times"""
        return [R.scaling_of(self.p, e, self.scaling, self.stride) for e in self.edges for _ in range(POINTS)]

    # the share-vector operations of NoirUltraHonkProver that the relations use
    def add(self, x, y):
        return [tuple((a + b) % self.p for a, b in zip(s, t)) for s, t in zip(x, y)]

    def sub(self, x, y):
        return [tuple((a - b) % self.p for a, b in zip(s, t)) for s, t in zip(x, y)]

    def scale(self, x, pub):
        """mul_with_public_many; `pub` a vector or a constant"""
        pub = pub if isinstance(pub, list) else [pub] * len(x)
        return [tuple(a * k % self.p for a in s) for s, k in zip(x, pub)]

    def add_pub(self, x, pub):
        """add_with_public_many / add_scalar: x (+) pub"""
        pub = pub if isinstance(pub, list) else [pub] * len(x)
        if self.pc is None:
            return list(x)
        return [tuple((a + k) % self.p if cc == self.pc else a for cc, a in enumerate(s)) for s, k in zip(x, pub)]

    def unflat(self, flat):
        nc = self.ncomp
        return [tuple(flat[i * nc:(i + 1) * nc]) for i in range(len(flat) // nc)]


def flat(vec):
    return [a for s in vec for a in s]


def fold(p, vec, length):
    """fold_accumulator! into a zero accumulator: entry k = the sum of the elements 7 j + k, cut to `length`. -> flat"""
    nc = len(vec[0]) if vec else None
    if nc is None:
        return None
    acc = [[0] * nc for _ in range(POINTS)]
    for idx, s in enumerate(vec):
        for cc, a in enumerate(s):
            acc[idx % POINTS][cc] = (acc[idx % POINTS][cc] + a) % p
    return [a for s in acc[:length] for a in s]


def _fold(v, vec, length):
    return fold(v.p, vec, length) if vec else [0] * (length * v.ncomp)


# ---- arithmetic, ultra_arithmetic_relation.rs:88-239 ------------------------------------------------------------------------------------
def local_mul_vec(v, x, y, mask):
    """T::local_mul_vec: Rep3 a a' + a b' + b a' + mask (rep3/arithmetic.rs:132-146); protocol 0 the product of the shares"""
    p = v.p
    if v.protocol == 1:
        assert mask is not None and len(mask) == len(x)
        return [(s[0] * t[0] + s[0] * t[1] + s[1] * t[0] + mk) % p for s, t, mk in zip(x, y, mask)]
    assert mask is None
    return [s[0] * t[0] % p for s, t in zip(x, y)]


def arith(v, mask):
    """-> (r0: 6 ints, a half share; r1: 5 shares, flat)"""
    p = v.p
    w_l, w_r, w_o, w_4, w_4_shift, w_l_shift = (v.sh(c) for c in ("w_l", "w_r", "w_o", "w_4", "w_4_shift", "w_l_shift"))
    q_m, q_l, q_r, q_o, q_4, q_c, q_arith = (v.pub(c) for c in ("q_m", "q_l", "q_r", "q_o", "q_4", "q_c", "q_arith"))
    sf = v.sf()
    neg_half = -pow(2, -1, p) % p
    mul = local_mul_vec(v, w_l, w_r, mask)
    half = lambda q, w: [a * s[0] % p for a, s in zip(q, w)]          # mul_with_public_to_half_share
    tmp_l, tmp_r, tmp_o, tmp_4 = half(q_l, w_l), half(q_r, w_r), half(q_o, w_o), half(q_4, w_4)
    r0 = []
    for i in range(POINTS * v.m):
        tmp = mul[i] * q_m[i] % p * (q_arith[i] - 3) % p * neg_half % p
        tmp += tmp_l[i] + tmp_r[i] + tmp_o[i] + tmp_4[i]
        if v.protocol == 0 or v.party == 0:                           # add_assign_public_half_share
            tmp += q_c[i]
        tmp += (q_arith[i] - 1) * w_4_shift[i][0]
        r0.append((tmp * q_arith[i] % p * sf[i] % p,))
    tmp = v.add_pub(v.sub(v.add(w_l, w_4), w_l_shift), q_m)
    tmp = v.scale(v.scale(v.scale(tmp, [(q - 2) % p for q in q_arith]), [(q - 1) % p for q in q_arith]), q_arith)
    tmp = v.scale(tmp, sf)
    return (fold(p, r0, 6) if r0 else [0] * 6), _fold(v, tmp, 5)


# ---- permutation, permutation_relation.rs:70-150, :202-249 --------------------------------------------------------------------------------
def perm_operands(v):
    """-> (lhs, rhs), 4 * 7 m shares each, flat"""
    beta, gamma, _ = v.params
    w = [v.sh(c) for c in ("w_l", "w_r", "w_o", "w_4")]
    wid = [v.add_pub(w[k], [(x * beta + gamma) % v.p for x in v.pub("id_%d" % (k + 1))]) for k in range(4)]
    wsigma = [v.add_pub(w[k], [(x * beta + gamma) % v.p for x in v.pub("sigma_%d" % (k + 1))]) for k in range(4)]
    return flat(wid[0] + wsigma[0] + wid[2] + wsigma[2]), flat(wid[1] + wsigma[1] + wid[3] + wsigma[3])


def perm_operands2(v):
    """-> rhs, 2 * 7 m shares, flat"""
    pid = v.params[2]
    tmp_lhs = v.add_pub(v.sh("z_perm"), v.pub("lagrange_first"))
    tmp_rhs = v.add_pub(v.sh("z_perm_shift"), [x * pid % v.p for x in v.pub("lagrange_last")])
    return flat(tmp_lhs + tmp_rhs)


def perm_finish(v, prod):
    """prod = mul_many([numerator | denominator], rhs). -> r0 (6) and r1 (3), back to back, flat"""
    mul1 = v.unflat(prod)
    half = len(mul1) >> 1
    tmp = v.scale(v.sub(mul1[:half], mul1[half:]), v.sf())
    tmp1 = v.scale(v.scale(v.sh("z_perm_shift"), v.pub("lagrange_last")), v.sf())
    return _fold(v, tmp, 6) + _fold(v, tmp1, 3)


# ---- delta range, delta_range_constraint_relation.rs:126-216 ------------------------------------------------------------------------------
def delta_operands(v):
    """-> lhs, 8 * 7 m shares, flat"""
    w_1, w_2, w_3, w_4, w_1_shift = (v.sh(c) for c in ("w_l", "w_r", "w_o", "w_4", "w_l_shift"))
    deltas = [v.sub(w_2, w_1), v.sub(w_3, w_2), v.sub(w_4, w_3), v.sub(w_1_shift, w_4)]
    lhs = []
    for c in (1, 2):
        for d in deltas:
            lhs += v.add_pub(d, (-c) % v.p)
    return flat(lhs)


def delta_sub_one(v, sqr):
    """add_assign_public(-1) on every element"""
    return flat(v.add_pub(v.unflat(sqr), v.p - 1))


def delta_finish(v, mul):
    """mul = mul_many of the two halves of the squares, 4 * 7 m shares. -> r0 .. r3 (6 each), flat"""
    mul = v.unflat(mul)
    n7 = POINTS * v.m
    q, sf = v.pub("q_delta_range") * 4, v.sf() * 4                     # cycled
    mul = v.scale(v.scale(mul, q), sf)
    return [a for i in range(4) for a in _fold(v, mul[i * n7:(i + 1) * n7], 6)]


# ---- lookup, logderiv_lookup_relation.rs:77-168, :255-312 -----------------------------------------------------------------------------------
def _write_term(v):
    beta, gamma, _ = v.params
    t = [v.pub("table_%d" % k) for k in (1, 2, 3, 4)]
    return [(a + gamma + b * beta + c * beta * beta + d * beta ** 3) % v.p for a, b, c, d in zip(*t)]


def _inverse_exists(v):
    row_has_write, row_has_read = v.sh("lookup_read_tags"), v.pub("q_lookup")
    res = v.scale(v.scale(row_has_write, row_has_read), v.p - 1)
    return v.add_pub(v.add(res, row_has_write), row_has_read)


def lookup_operands(v):
    """-> (read_term, the extended lookup_inverses), 7 m shares each, flat"""
    beta, gamma, _ = v.params
    p = v.p
    d1 = v.add_pub(v.add(v.scale(v.sh("w_l_shift"), v.pub("q_r")), v.sh("w_l")), gamma)
    d2 = v.scale(v.add(v.scale(v.sh("w_r_shift"), v.pub("q_m")), v.sh("w_r")), beta)
    d3 = v.scale(v.add(v.scale(v.sh("w_o_shift"), v.pub("q_c")), v.sh("w_o")), beta * beta % p)
    d1 = v.add(v.add(d1, d2), d3)
    d1 = v.add_pub(d1, [x * pow(beta, 3, p) % p for x in v.pub("q_o")])
    return flat(d1), flat(v.sh("lookup_inverses"))


def lookup_mid(v, write_inverse):
    """write_inverse = mul_many(read_term, inverses). -> (r0 (5), lhs = [write_inverse | read_tag], rhs = [read_counts | read_tag]), flat"""
    wi = v.unflat(write_inverse)
    tmp = v.scale(v.sub(v.scale(wi, _write_term(v)), _inverse_exists(v)), v.sf())
    tag = v.sh("lookup_read_tags")
    return _fold(v, tmp, 5), flat(wi + tag), flat(v.sh("lookup_read_counts") + tag)


def lookup_finish(v, mul):
    """mul = mul_many(lhs, rhs). -> r1 (5, no scaling) and r2 (3), back to back, flat"""
    mul = v.unflat(mul)
    half = len(mul) >> 1
    read_inverse = v.scale(v.sh("lookup_inverses"), _write_term(v))
    tmp = v.sub(v.scale(read_inverse, v.pub("q_lookup")), mul[:half])
    tmp2 = v.scale(v.sub(mul[half:], v.sh("lookup_read_tags")), v.sf())
    return _fold(v, tmp, 5) + _fold(v, tmp2, 3)


# ---- the plain side --------------------------------------------------------------------------------------------------------------------------
def plain_accumulate(p, polys, edge_begin, edge_end, scaling, stride, params):
    """R.accumulate_range with the skips the shared prover has: arith and delta by their selector, perm and lookup never"""
    acc = [[0] * ln for ln in R.ACC_LEN]
    for e in range(edge_begin, edge_end, 2):
        sf = R.scaling_of(p, e, scaling, stride)
        for rel in ("arith", "perm", "delta", "lookup"):
            for s, c in zip(R.RELATION_OF[rel], R.edge_contribution(p, polys, e, params, sf, rel, honour_skip=rel in ("arith", "delta"))):
                acc[s] = [(a + b) % p for a, b in zip(acc[s], c)]
    return acc


def one_end_edges_count(p, polys, col, rel, edge_begin, edge_end, scaling, stride, params):
    """the edges whose selector `col` is zero at exactly one end; asserts that each adds a non-zero value to every subrelation of `rel`"""
    out = []
    for e in range(edge_begin, edge_end, 2):
        if bool(polys[col][e]) != bool(polys[col][e + 1]):
            c = R.edge_contribution(p, polys, e, params, R.scaling_of(p, e, scaling, stride), rel)
            assert all(any(a) for a in c), (rel, e)
            out.append(e)
    return out


# ---- sharing and the in-process networks ------------------------------------------------------------------------------------------------
def share_polys(p, polys, kind, rnd):
    """-> the three parties' column dicts (kind "rep3" or "shamir") or the one party's (kind "plain"); public columns are shared objects"""
    n_parties = 1 if kind == "plain" else 3
    out = [dict() for _ in range(n_parties)]
    for c, vals in polys.items():
        if c not in SHARED or kind == "plain":
            for o in out:
                o[c] = vals
            continue
        cols = [[] for _ in range(3)]
        for x in vals:
            if kind == "rep3":
                a, b = rnd.randrange(p), rnd.randrange(p)
                cc = (x - a - b) % p
                for i, s in enumerate(((a, cc), (b, a), (cc, b))):     # party i holds (x_i, x_(i-1))
                    cols[i] += s
            else:
                r1 = rnd.randrange(p)
                for i in range(3):
                    cols[i].append((x + r1 * (i + 1)) % p)
        for o, col in zip(out, cols):
            o[c] = col
    return out


class PlainNet:
    kind, protocol, n = "plain", 0, 1

    def __init__(self, p, rnd=None, local_mul=None):
        self.p, self.local_mul = p, local_mul or (lambda i, x, y, mask: [a * b % p for a, b in zip(x, y)])

    def masks(self, n):
        return [None]

    def mul_many(self, lhs, rhs):
        return [self.local_mul(0, lhs[0], rhs[0], None)]

    def reshare(self, halves):
        return halves

    def open(self, shares):
        return list(shares[0])


class Rep3Net:
    """three parties; local_mul(i, lhs, rhs, mask) -> party i's half shares; the harness rotates them (reshare: send to the next party,
    receive from the previous one, rep3/arithmetic.rs:148-161)"""
    kind, protocol, n = "rep3", 1, 3

    def __init__(self, p, rnd, local_mul=None):
        self.p, self.rnd = p, rnd
        self.local_mul = local_mul or (lambda i, x, y, mask: [(x[2 * k] * (y[2 * k] + y[2 * k + 1]) + x[2 * k + 1] * y[2 * k] + mask[k]) % p
                                                               for k in range(len(mask))])

    def masks(self, n):
        """correlated randomness: the three vectors add up to zero"""
        m0, m1 = [self.rnd.randrange(self.p) for _ in range(n)], [self.rnd.randrange(self.p) for _ in range(n)]
        return [m0, m1, [(-a - b) % self.p for a, b in zip(m0, m1)]]

    def mul_many(self, lhs, rhs):
        masks = self.masks(len(lhs[0]) // 2)
        return self.reshare([self.local_mul(i, lhs[i], rhs[i], masks[i]) for i in range(3)])

    def reshare(self, halves):
        return [[c for own, prev in zip(halves[i], halves[(i + 2) % 3]) for c in (own, prev)] for i in range(3)]

    def open(self, shares):
        return [(shares[0][2 * k] + shares[1][2 * k] + shares[2][2 * k]) % self.p for k in range(len(shares[0]) // 2)]


class ShamirNet:
    """three parties at the points 1, 2, 3, degree 1; a product has degree 2 and is reduced by open-and-reshare (test-only)"""
    kind, protocol, n = "shamir", 0, 3

    def __init__(self, p, rnd, local_mul=None):
        self.p, self.rnd = p, rnd
        self.local_mul = local_mul or (lambda i, x, y, mask: [a * b % p for a, b in zip(x, y)])
        self.lagrange = [3, p - 3, 1]                                  # the value at 0 of a polynomial of degree <= 2 through 1, 2, 3

    def masks(self, n):
        return [None] * 3

    def mul_many(self, lhs, rhs):
        return self.reshare([self.local_mul(i, lhs[i], rhs[i], None) for i in range(3)])

    def reshare(self, halves):
        out = [[], [], []]
        for x in self.open(halves):
            r1 = self.rnd.randrange(self.p)
            for i in range(3):
                out[i].append((x + r1 * (i + 1)) % self.p)
        return out

    def open(self, shares):
        return [sum(l * s[k] for l, s in zip(self.lagrange, shares)) % self.p for k in range(len(shares[0]))]


NETS = {"plain": PlainNet, "rep3": Rep3Net, "shamir": ShamirNet}


class RefStages:
    """the stage functions of this module over the parties' views: views[rel][party]"""

    def __init__(self, views):
        self.views = views

    def m(self, rel):
        return self.views[rel][0].m

    def arith(self, i, mask):
        return arith(self.views["arith"][i], mask)

    def perm_operands(self, i):
        return perm_operands(self.views["perm"][i])

    def perm_operands2(self, i):
        return perm_operands2(self.views["perm"][i])

    def perm_finish(self, i, prod):
        return perm_finish(self.views["perm"][i], prod)

    def delta_operands(self, i):
        return delta_operands(self.views["delta"][i])

    def delta_sub_one(self, i, sqr):
        return delta_sub_one(self.views["delta"][i], sqr)

    def delta_finish(self, i, mul):
        return delta_finish(self.views["delta"][i], mul)

    def lookup_operands(self, i):
        return lookup_operands(self.views["lookup"][i])

    def lookup_mid(self, i, wi):
        return lookup_mid(self.views["lookup"][i], wi)

    def lookup_finish(self, i, mul):
        return lookup_finish(self.views["lookup"][i], mul)


class Both:
    """runs every stage on two sets of stage functions and asserts equal outputs, word for word; hands on the first's"""

    def __init__(self, ref, other):
        self.ref, self.other = ref, other
        self.compared = 0

    def m(self, rel):
        return self.ref.m(rel)

    def __getattr__(self, name):
        def stage(i, *args):
            want, got = getattr(self.ref, name)(i, *args), getattr(self.other, name)(i, *args)
            norm = lambda x: [norm(y) for y in x] if isinstance(x, (list, tuple)) else x
            assert norm(got) == norm(want), (name, "party", i)
            self.compared += 1
            return want
        return stage


PLANTS = (("arith.skip", "q_arith"), ("arith.one_end", "q_arith"), ("delta.skip", "q_delta_range"), ("delta.one_end", "q_delta_range"))


def random_case(p, n, seed):
    """n elements per column of random (unsatisfied) non-zero data, so that every term counts and no edge meets the plain skips of perm and
    lookup (asserted). Planted from the last edge down, edge 0 left alone: for q_arith and q_delta_range one edge with zero at both ends
    (left out) and one with zero at the first end only (kept). -> dict(n, polys, params, betas, planted: name -> edge index)"""
    import random
    r = random.Random(seed)
    polys = {c: [r.randrange(1, p) for _ in range(n)] for c in R.COLS}
    edges, planted = n // 2, {}
    for i, (name, col) in enumerate(PLANTS):
        if i + 1 < edges:
            e = 2 * (edges - 1 - i)
            polys[col][e] = 0
            if name.endswith("skip"):
                polys[col][e + 1] = 0
            planted[name] = e
    for e in range(0, n, 2):
        ext = R.extend_edges(p, polys, e)
        assert not R.skip_perm(ext) and not R.skip_lookup(ext), "no edge meets a skip that only the plain prover has"
    return dict(n=n, polys=polys, params=tuple(r.randrange(1, p) for _ in range(3)), betas=[r.randrange(1, p) for _ in range(12)], planted=planted)


def table_of(p, c, stride):
    """the gate-separator products that reach every edge of the case at this stride"""
    return R.beta_products(p, c["betas"], max(1, ((c["n"] // 2 - 1) * stride).bit_length()))


def make_views(p, party_polys, protocol, params, edge_begin, edge_end, scaling=None, stride=1, lists=None):
    """views[rel][party]; arith and delta take the edge lists of their selectors (lists: rel -> list, else selected here)"""
    pub = party_polys[0]
    lists = lists or {"arith": select_edges(pub, "q_arith", edge_begin, edge_end), "delta": select_edges(pub, "q_delta_range", edge_begin, edge_end)}
    return {rel: [View(p, polys, protocol, i, params, edge_begin, edge_end, lists.get(rel), scaling, stride) for i, polys in enumerate(party_polys)]
            for rel in ("arith", "perm", "delta", "lookup")}


def halves(vec):
    return vec[:len(vec) >> 1], vec[len(vec) >> 1:]


def run_round(net, st):
    """accumulate_relation_univariates_batch (co_sumcheck_round.rs:140-218) for the four relations + the reshare of arith.r0 (:292), every
    party in turn. -> per party the eleven accumulators (flat share lists) in subrelation order"""
    P = range(net.n)
    masks = net.masks(POINTS * st.m("arith")) if st.m("arith") else [None if net.protocol == 0 else [] for _ in P]
    ar = [st.arith(i, masks[i]) for i in P]
    r0 = net.reshare([a[0] for a in ar])
    acc = [[r0[i], ar[i][1]] for i in P]
    # permutation
    ops = [st.perm_operands(i) for i in P]
    mul1 = net.mul_many([o[0] for o in ops], [o[1] for o in ops])
    num_den = net.mul_many([halves(x)[0] for x in mul1], [halves(x)[1] for x in mul1])
    prod = net.mul_many(num_den, [st.perm_operands2(i) for i in P])
    for i in P:
        out, nc = st.perm_finish(i, prod[i]), net.protocol + 1
        acc[i] += [out[:6 * nc], out[6 * nc:]]
    # delta range
    if st.m("delta"):
        lhs = [st.delta_operands(i) for i in P]
        sqr = net.mul_many(lhs, lhs)
        sqr = [st.delta_sub_one(i, sqr[i]) for i in P]
        mul = net.mul_many([halves(x)[0] for x in sqr], [halves(x)[1] for x in sqr])
    else:
        mul = [[] for _ in P]
    delta = [st.delta_finish(i, mul[i]) for i in P]
    # lookup
    ops = [st.lookup_operands(i) for i in P]
    wi = net.mul_many([o[0] for o in ops], [o[1] for o in ops])
    mid = [st.lookup_mid(i, wi[i]) for i in P]
    mul = net.mul_many([x[1] for x in mid], [x[2] for x in mid])
    for i in P:
        out, nc = st.lookup_finish(i, mul[i]), net.protocol + 1
        acc[i] += [mid[i][0], out[:5 * nc], out[5 * nc:]]
        acc[i] += [delta[i][6 * nc * k:6 * nc * (k + 1)] for k in range(4)]
    return acc


def open_round(net, acc):
    """-> the eleven opened accumulators"""
    return [net.open([acc[i][s] for i in range(net.n)]) for s in range(len(R.ACC_LEN))]


def batch_over_relations_shares(p, acc, ncomp, pc, alphas, current_element, partial_evaluation_result):
    """batch_over_relations_univariates on one party's shares (co_sumcheck_round.rs:121-138; relations/mod.rs `scale` and
    extend_and_batch_univariates on SharedUnivariate): linear in the shares, so component by component. -> 8 shares, flat"""
    out = [0] * (R.BATCHED_RELATION_PARTIAL_LENGTH * ncomp)
    for cc in range(ncomp):
        res = R.batch_over_relations_univariates(p, [a[cc::ncomp] for a in acc], alphas, current_element, partial_evaluation_result)
        out[cc::ncomp] = res
    return out
