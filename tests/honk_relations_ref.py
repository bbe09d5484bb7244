"""The loop between two folds of co-noir's UltraHonk sumcheck prover, restated in Python integers from the PROVER side of the reference:
SumcheckProverRound::compute_univariate_inner with extend_edges and the per-relation skips
(co-noir/ultrahonk/src/decider/sumcheck/sumcheck_round_prover.rs:124-255), the `accumulate` bodies over univariates of length 7 of
UltraArithmeticRelation (relations/ultra_arithmetic_relation.rs:126-175), UltraPermutationRelation (permutation_relation.rs:93-167),
LogDerivLookupRelation (logderiv_lookup_relation.rs:77-126, :164-183, :266-309) and DeltaRangeConstraintRelation
(delta_range_constraint_relation.rs:112-177), truncated to the accumulator lengths, GateSeparatorPolynomial (decider/types.rs:53-112) and
batch_over_relations_univariates (:76-122, relations/mod.rs:134-199, univariate.rs:57-178, :215-230). The device's per-point functions are
written from the scalar verify_accumulate bodies; `relations_at_point` below restates those too, so that the two shapes can be compared
without a device. Also what the CPU and the GPU tests share: a satisfied trace in closed form and a random case with planted skip edges."""
import functools
import random

from tests import honk_oink_ref as OINK

MAX_PARTIAL_RELATION_LENGTH = 7
BATCHED_RELATION_PARTIAL_LENGTH = 8
WITNESS = ["w_l", "w_r", "w_o", "w_4", "z_perm", "lookup_inverses", "lookup_read_counts", "lookup_read_tags"]
SHIFTED = ["w_l_shift", "w_r_shift", "w_o_shift", "w_4_shift", "z_perm_shift"]
PRECOMPUTED = ["q_m", "q_c", "q_l", "q_r", "q_o", "q_4", "q_arith", "q_delta_range", "q_lookup", "sigma_1", "sigma_2", "sigma_3", "sigma_4",
               "id_1", "id_2", "id_3", "id_4", "table_1", "table_2", "table_3", "table_4", "lagrange_first", "lagrange_last"]
COLS = WITNESS + SHIFTED + PRECOMPUTED          # the order of cols_dev
SUBRELATIONS = ["arith.r0", "arith.r1", "perm.r0", "perm.r1", "lookup.r0", "lookup.r1", "lookup.r2", "delta.r0", "delta.r1", "delta.r2", "delta.r3"]
ACC_LEN = [6, 5, 6, 3, 5, 5, 3, 6, 6, 6, 6]      # the reference's accumulator lengths
RELATION_OF = {"arith": [0, 1], "perm": [2, 3], "lookup": [4, 5, 6], "delta": [7, 8, 9, 10]}
LINEARLY_DEPENDENT = 5                           # lookup.r1: no scaling factor, no gate-separator factor
assert len(COLS) == 36 and sum(ACC_LEN) == 57


class Uni:
    """Univariate<F, SIZE> by its evaluations at 0 .. SIZE - 1; an int operand is a field constant (added to / multiplied into every
    evaluation, as the reference's `Univariate + &F` and `Univariate * &F` do)"""

    def __init__(self, p, ev):
        self.p, self.ev = p, [v % p for v in ev]

    def _other(self, o):
        return o.ev if isinstance(o, Uni) else [o] * len(self.ev)

    def __add__(self, o):
        return Uni(self.p, [a + b for a, b in zip(self.ev, self._other(o))])

    def __sub__(self, o):
        return Uni(self.p, [a - b for a, b in zip(self.ev, self._other(o))])

    def __mul__(self, o):
        return Uni(self.p, [a * b for a, b in zip(self.ev, self._other(o))])

    def __neg__(self):
        return Uni(self.p, [-a for a in self.ev])

    def sqr(self):
        return self * self

    def is_zero(self):
        return not any(self.ev)


def extend_from(p, poly, size):
    """Univariate::extend_from, univariate.rs:57-178. Two points: the running sum of the reference. Longer inputs: the reference's three
    other branches (closed forms for 3 and 4 points, barycentric beyond) all evaluate the one polynomial of degree < len(poly) through the
    points 0 .. len(poly) - 1, computed here by Lagrange's formula."""
    ev = [v % p for v in poly]
    ln = len(ev)
    assert 2 <= ln <= size
    if ln == 2:
        delta = (ev[1] - ev[0]) % p
        for _ in range(ln, size):
            ev.append((ev[-1] + delta) % p)
        return ev
    return ev + [lagrange_eval(p, poly, x) for x in range(ln, size)]


def lagrange_eval(p, evals, x):
    """the polynomial of degree < len(evals) through (i, evals[i]) at x"""
    total = 0
    for i, v in enumerate(evals):
        num = den = 1
        for j in range(len(evals)):
            if j != i:
                num = num * (x - j) % p
                den = den * (i - j) % p
        total += v * num % p * pow(den, -1, p)
    return total % p


def extend_edges(p, polys, edge_idx):
    """extend_edges: every column's pair -> a univariate of length 7"""
    return {c: Uni(p, extend_from(p, [polys[c][edge_idx], polys[c][edge_idx + 1]], MAX_PARTIAL_RELATION_LENGTH)) for c in COLS}


# ---- skip, prover side ----------------------------------------------------------------------------------------------------------------------
def skip_arith(e):
    return e["q_arith"].is_zero()


def skip_perm(e):
    return (e["z_perm"] - e["z_perm_shift"]).is_zero()


def skip_lookup(e):
    return e["q_lookup"].is_zero() and e["lookup_read_counts"].is_zero()


def skip_delta(e):
    return e["q_delta_range"].is_zero()


SKIP = {"arith": skip_arith, "perm": skip_perm, "lookup": skip_lookup, "delta": skip_delta}


# ---- accumulate, prover side: -> the univariates (length 7) that are added to r0, r1, ... ------------------------------------------------
def accumulate_arith(p, e, params, sf):
    neg_half = -pow(2, -1, p) % p
    tmp = (e["q_arith"] - 3) * (e["q_m"] * e["w_r"] * e["w_l"]) * neg_half
    tmp = tmp + ((e["q_l"] * e["w_l"]) + (e["q_r"] * e["w_r"]) + (e["q_o"] * e["w_o"]) + (e["q_4"] * e["w_4"]) + e["q_c"])
    tmp = tmp + (e["q_arith"] - 1) * e["w_4_shift"]
    tmp = tmp * e["q_arith"]
    r0 = tmp * sf
    tmp = e["w_l"] + e["w_4"] - e["w_l_shift"] + e["q_m"]
    tmp = tmp * (e["q_arith"] - 2)
    tmp = tmp * (e["q_arith"] - 1)
    tmp = tmp * e["q_arith"]
    return [r0, tmp * sf]


def accumulate_perm(p, e, params, sf):
    beta, gamma, public_input_delta = params
    wg = [e[w] + gamma for w in ("w_l", "w_r", "w_o", "w_4")]
    t1 = (e["id_1"] * beta + wg[0]) * sf
    for k in (1, 2, 3):
        t1 = t1 * (e["id_%d" % (k + 1)] * beta + wg[k])
    t5 = (e["sigma_1"] * beta + wg[0]) * sf
    for k in (1, 2, 3):
        t5 = t5 * (e["sigma_%d" % (k + 1)] * beta + wg[k])
    public_input_term = e["lagrange_last"] * public_input_delta + e["z_perm_shift"]
    r0 = ((e["z_perm"] + e["lagrange_first"]) * t1) - (public_input_term * t5)
    r1 = (e["lagrange_last"] * e["z_perm_shift"]) * sf
    return [r0, r1]


def lookup_terms(p, e, params):
    beta, gamma, _ = params
    beta_sqr, beta_cube = beta * beta % p, beta * beta * beta % p
    row_has_write, row_has_read = e["lookup_read_tags"], e["q_lookup"]
    inverse_exists = -(row_has_write * row_has_read) + row_has_write + row_has_read
    derived_1 = e["w_l"] + gamma + e["q_r"] * e["w_l_shift"]
    derived_2 = e["q_m"] * e["w_r_shift"] + e["w_r"]
    derived_3 = e["q_c"] * e["w_o_shift"] + e["w_o"]
    read_term = derived_1 + derived_2 * beta + derived_3 * beta_sqr + e["q_o"] * beta_cube
    write_term = e["table_1"] + gamma + e["table_2"] * beta + e["table_3"] * beta_sqr + e["table_4"] * beta_cube
    return inverse_exists, read_term, write_term


def accumulate_lookup(p, e, params, sf):
    inverses, read_counts, read_selector = e["lookup_inverses"], e["lookup_read_counts"], e["q_lookup"]
    inverse_exists, read_term, write_term = lookup_terms(p, e, params)
    write_inverse = read_term * inverses
    read_inverse = write_term * inverses
    r0 = (read_term * write_term * inverses - inverse_exists) * sf
    r1 = read_inverse * read_selector - write_inverse * read_counts          # no scaling factor
    read_tag = e["lookup_read_tags"]
    r2 = (read_tag * read_tag - read_tag) * sf
    return [r0, r1, r2]


def accumulate_delta(p, e, params, sf):
    minus_one, minus_two = p - 1, p - 2
    deltas = [e["w_r"] - e["w_l"], e["w_o"] - e["w_r"], e["w_4"] - e["w_o"], e["w_l_shift"] - e["w_4"]]
    out = []
    for d in deltas:
        tmp = (d + minus_one).sqr() + minus_one
        tmp = tmp * ((d + minus_two).sqr() + minus_one)
        tmp = tmp * e["q_delta_range"]
        out.append(tmp * sf)
    return out


ACCUMULATE = {"arith": accumulate_arith, "perm": accumulate_perm, "lookup": accumulate_lookup, "delta": accumulate_delta}


def edge_contribution(p, polys, edge_idx, params, sf, relation, honour_skip=True):
    """what one edge adds to the relation's accumulators (truncated to their lengths); all zeros when the edge is skipped"""
    e = extend_edges(p, polys, edge_idx)
    idx = RELATION_OF[relation]
    if honour_skip and SKIP[relation](e):
        return [[0] * ACC_LEN[s] for s in idx]
    return [u.ev[:ACC_LEN[s]] for s, u in zip(idx, ACCUMULATE[relation](p, e, params, sf))]


def scaling_of(p, edge_idx, scaling, stride):
    return 1 if scaling is None else scaling[(edge_idx >> 1) * stride]


def accumulate_range(p, polys, edge_begin, edge_end, scaling, stride, params, honour_skip=True):
    """the loop of compute_univariate_inner over (edge_begin..edge_end).step_by(2) -> the eleven accumulators"""
    acc = [[0] * ln for ln in ACC_LEN]
    for edge_idx in range(edge_begin, edge_end, 2):
        sf = scaling_of(p, edge_idx, scaling, stride)
        for relation in ("arith", "perm", "delta", "lookup"):       # the reference's order; sums do not depend on it
            for s, c in zip(RELATION_OF[relation], edge_contribution(p, polys, edge_idx, params, sf, relation, honour_skip)):
                acc[s] = [(a + b) % p for a, b in zip(acc[s], c)]
    return acc


def flat_acc(acc):
    return [v for a in acc for v in a]


# ---- the scalar shape (verify_accumulate), for the comparison of the two shapes -----------------------------------------------------------
def relations_at_point(p, v, params, sf):
    """v: column name -> value at one point. -> the eleven subrelation values"""
    beta, gamma, pid = params
    qa = v["q_arith"]
    t = (qa - 3) * (v["q_m"] * v["w_r"] * v["w_l"]) * (-pow(2, -1, p))
    t += v["q_l"] * v["w_l"] + v["q_r"] * v["w_r"] + v["q_o"] * v["w_o"] + v["q_4"] * v["w_4"] + v["q_c"] + (qa - 1) * v["w_4_shift"]
    out = [t * qa * sf, (v["w_l"] + v["w_4"] - v["w_l_shift"] + v["q_m"]) * (qa - 2) * (qa - 1) * qa * sf]
    num = den = sf
    for k, w in enumerate(("w_l", "w_r", "w_o", "w_4")):
        num = num * (v["id_%d" % (k + 1)] * beta + v[w] + gamma) % p
        den = den * (v["sigma_%d" % (k + 1)] * beta + v[w] + gamma) % p
    out += [(v["z_perm"] + v["lagrange_first"]) * num - (v["lagrange_last"] * pid + v["z_perm_shift"]) * den, v["lagrange_last"] * v["z_perm_shift"] * sf]
    b2, b3 = beta * beta % p, beta * beta * beta % p
    read = v["w_l"] + gamma + v["q_r"] * v["w_l_shift"] + (v["q_m"] * v["w_r_shift"] + v["w_r"]) * beta + (v["q_c"] * v["w_o_shift"] + v["w_o"]) * b2 + v["q_o"] * b3
    write = v["table_1"] + gamma + v["table_2"] * beta + v["table_3"] * b2 + v["table_4"] * b3
    tag, ql, inv = v["lookup_read_tags"], v["q_lookup"], v["lookup_inverses"]
    out += [(read * write * inv - (tag + ql - tag * ql)) * sf, write * inv * ql - read * inv * v["lookup_read_counts"], (tag * tag - tag) * sf]
    for hi, lo in (("w_r", "w_l"), ("w_o", "w_r"), ("w_4", "w_o"), ("w_l_shift", "w_4")):
        d = v[hi] - v[lo]
        out.append(((d - 1) ** 2 - 1) * ((d - 2) ** 2 - 1) * v["q_delta_range"] * sf)
    return [x % p for x in out]


# ---- the gate separator, decider/types.rs:44-112 --------------------------------------------------------------------------------------------
def beta_products(p, betas, log_num_monomials):
    out = [1] * (1 << log_num_monomials)
    for i, beta in enumerate(betas[:log_num_monomials]):
        index = 1 << i
        out[index] = beta
        for j in range(1, index):
            out[index + j] = out[j] * beta % p
    return out


class GateSeparator:
    def __init__(self, p, betas, log_num_monomials):
        self.p, self.betas = p, list(betas)
        self.beta_products = beta_products(p, betas, log_num_monomials)
        self.partial_evaluation_result, self.current_element_idx, self.periodicity = 1, 0, 2

    def current_element(self):
        return self.betas[self.current_element_idx]

    def partially_evaluate(self, u):
        self.partial_evaluation_result = self.partial_evaluation_result * (1 + u * (self.betas[self.current_element_idx] - 1)) % self.p
        self.current_element_idx += 1
        self.periodicity *= 2


def batch_over_relations_univariates(p, acc, alphas, current_element, partial_evaluation_result, size=BATCHED_RELATION_PARTIAL_LENGTH):
    """AllRelationAcc::scale with first_scalar = 1 and alphas[0..10), then extend_and_batch_univariates, for subrelations 0 .. 10"""
    assert len(alphas) == 10
    scalars = [1] + list(alphas)
    extended_random = extend_from(p, [1, current_element], size)
    result = [0] * size
    for s, a in enumerate(acc):
        ext = extend_from(p, [v * scalars[s] % p for v in a], size)
        for i in range(size):
            if s == LINEARLY_DEPENDENT:
                result[i] = (result[i] + ext[i]) % p
            else:
                result[i] = (result[i] + ext[i] * extended_random[i] % p * partial_evaluation_result) % p
    return result


def fold(p, v, u):
    """partially_evaluate of one column: out[j] = v[2 j] + u (v[2 j + 1] - v[2 j])"""
    return [(v[2 * j] + u * (v[2 * j + 1] - v[2 * j])) % p for j in range(len(v) // 2)]


# ---- a satisfied trace in closed form ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def satisfied_trace(p):
    """n = 16, active rows 0 .. 12. Row 0 is empty; arithmetic gates with q_arith = 1 (rows 1, 6, 8), 2 (row 2) and 3 (row 4); a delta-range
    gate at row 5 (steps 1, 2, 3 and, into w_l of row 6, 0); a lookup read at row 7 of the table row 10; random copy cycles of length 1, 2,
    3 and 5 over the cells of rows 1 .. 11 that the delta-range gate leaves free. z_perm and lookup_inverses come from the Oink restatement.
    public_input_delta = 1 (no public inputs). -> dict(polys, params, n)"""
    r = random.Random(2025)
    n, last = 16, 12
    rnd = lambda: r.randrange(1, p)
    # wires and the permutation: the cells of the delta-range gate map to themselves, the others run in random cycles
    w = [[0] * n for _ in range(4)]
    ident = [[k * n + i for i in range(n)] for k in range(4)]
    sigma = [row[:] for row in ident]
    base = rnd()
    for k, step in enumerate((0, 1, 3, 6)):
        w[k][5] = (base + step) % p
    w[0][6] = (base + 6) % p
    reserved = {(k, 5) for k in range(4)} | {(0, 6)}
    cells = [(k, i) for k in range(4) for i in range(1, last) if (k, i) not in reserved]
    r.shuffle(cells)
    pos = 0
    while pos < len(cells):
        ln = min(len(cells) - pos, r.choice([1, 2, 3, 5]))
        cyc, v = cells[pos:pos + ln], rnd()
        pos += ln
        for t, (k, i) in enumerate(cyc):
            w[k][i] = v
            k2, i2 = cyc[(t + 1) % ln]
            sigma[k][i] = ident[k2][i2]
    for k in range(4):
        w[k][last] = rnd()
    sel = {c: [0] * n for c in ("q_m", "q_c", "q_l", "q_r", "q_o", "q_4", "q_arith", "q_delta_range", "q_lookup")}
    half = pow(2, -1, p)
    for row, qa in ((1, 1), (6, 1), (8, 1), (2, 2), (4, 3)):
        sel["q_arith"][row] = qa
        for c in ("q_l", "q_r", "q_o", "q_4"):
            sel[c][row] = rnd()
        sel["q_m"][row] = (w[0][row + 1] - w[0][row] - w[3][row]) % p if qa == 3 else rnd()
        lin = sum(sel[c][row] * w[k][row] for k, c in enumerate(("q_l", "q_r", "q_o", "q_4")))
        prod = (3 - qa) * half * sel["q_m"][row] * w[1][row] * w[0][row]
        sel["q_c"][row] = -(prod + lin + (qa - 1) * w[3][row + 1]) % p
    sel["q_delta_range"][5] = 1
    tables = [[rnd() for _ in range(n)] for _ in range(4)]
    gate, trow = 7, 10
    sel["q_lookup"][gate] = 1
    for c in ("q_r", "q_m", "q_c", "q_o"):
        sel[c][gate] = rnd()
    tables[0][trow] = (w[0][gate] + sel["q_r"][gate] * w[0][gate + 1]) % p
    tables[1][trow] = (w[1][gate] + sel["q_m"][gate] * w[1][gate + 1]) % p
    tables[2][trow] = (w[2][gate] + sel["q_c"][gate] * w[2][gate + 1]) % p
    tables[3][trow] = sel["q_o"][gate]
    counts, tags = [0] * n, [0] * n
    counts[trow] = tags[trow] = 1
    beta, gamma = rnd(), rnd()
    _, z_perm = OINK.grand_product_plain(p, n, w, ident, sigma, beta, gamma, last + 1, None)
    _, _, inverses = OINK.lookup_inverses_plain(p, w[0], w[1], w[2], tags, sel["q_r"], sel["q_m"], sel["q_c"], sel["q_o"], tables, sel["q_lookup"], beta, gamma)
    shift = lambda v: v[1:] + [0]
    polys = dict(sel)
    polys.update(w_l=w[0], w_r=w[1], w_o=w[2], w_4=w[3], z_perm=z_perm, lookup_inverses=inverses, lookup_read_counts=counts, lookup_read_tags=tags)
    polys.update(w_l_shift=shift(w[0]), w_r_shift=shift(w[1]), w_o_shift=shift(w[2]), w_4_shift=shift(w[3]), z_perm_shift=shift(z_perm))
    for k in range(4):
        polys["sigma_%d" % (k + 1)], polys["id_%d" % (k + 1)], polys["table_%d" % (k + 1)] = sigma[k], ident[k], tables[k]
    polys["lagrange_first"] = [1] + [0] * (n - 1)
    polys["lagrange_last"] = [1 if i == last else 0 for i in range(n)]
    assert set(polys) == set(COLS)
    return dict(n=n, polys=polys, params=(beta, gamma, 1), w=w, ident=ident, sigma=sigma, tables=tables, tags=tags, last=last)


def check_round_chain(p, n, betas, alphas, challenges, accumulators_of_round, fold_all):
    """The sumcheck identities of a satisfied trace over log2(n) rounds. accumulators_of_round(round, size, gate_separator) -> the eleven
    accumulators of the current columns; fold_all(u) folds every column. Asserts: in round 0 entries 0 and 1 of every accumulator but
    lookup.r1 are zero and lookup.r1[0] + lookup.r1[1] = 0; S(0) + S(1) = 0 in round 0; S'(0) + S'(1) = S(u) afterwards."""
    log_n = n.bit_length() - 1
    gs = GateSeparator(p, betas, log_n)
    target, size = 0, n
    for rnd in range(log_n):
        acc = accumulators_of_round(rnd, size, gs)
        if rnd == 0:
            for s, a in enumerate(acc):
                if s == LINEARLY_DEPENDENT:
                    assert (a[0] + a[1]) % p == 0 and a[0] != 0, "lookup.r1 sums to zero over the trace, and is not trivially zero"
                else:
                    assert a[0] == 0 and a[1] == 0, (SUBRELATIONS[s], "vanishes on every row of a satisfied trace")
        S = batch_over_relations_univariates(p, acc, alphas, gs.current_element(), gs.partial_evaluation_result)
        assert (S[0] + S[1]) % p == target, ("round", rnd)
        assert any(S[2:]), "the round univariate is not trivially zero"
        u = challenges[rnd]
        target = lagrange_eval(p, S, u)
        gs.partially_evaluate(u)
        fold_all(u)
        size >>= 1
    return target


# ---- a random case with planted skip edges ---------------------------------------------------------------------------------------------------
PLANTS = ["perm.skip", "lookup.skip", "perm.one_end", "lookup.one_end", "arith.skip", "arith.one_end", "delta.skip", "delta.one_end"]


def random_case(p, n, seed, plants=True):
    """n elements per column of random (unsatisfied) data, every term non-zero. Planted from the last edge down, edge 0 left alone: for each
    skip predicate one edge where it holds at both ends (left out) and one where it holds at the first end only (counted).
    -> dict(polys, params, planted: name -> edge_idx)"""
    r = random.Random(seed)
    polys = {c: [r.randrange(1, p) for _ in range(n)] for c in COLS}
    params = tuple(r.randrange(1, p) for _ in range(3))
    planted = {}
    edges = n // 2
    for i, name in enumerate(PLANTS[:max(0, edges - 1)] if plants else []):
        e = 2 * (edges - 1 - i)
        ends = (e, e + 1) if name.endswith(".skip") else (e,)
        for x in ends:
            if name.startswith("arith"):
                polys["q_arith"][x] = 0
            elif name.startswith("delta"):
                polys["q_delta_range"][x] = 0
            elif name.startswith("perm"):
                polys["z_perm_shift"][x] = polys["z_perm"][x]
            else:
                polys["q_lookup"][x] = polys["lookup_read_counts"][x] = 0
        planted[name] = e
    return dict(n=n, polys=polys, params=params, planted=planted)
