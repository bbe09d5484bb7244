"""The Oink loops of co-noir's UltraHonk prover that run over the whole trace, restated in Python integers loop for loop from
co-noir/co-ultrahonk/src/co_oink/co_oink_prover.rs: add_ram_rom_memory_records_to_wire_4 (:98-160), compute_logderivative_inverses with
compute_lookup_term and compute_table_term (:162-293), batched_grand_product_num_denom (:344-451) and the sequential placement and fill
loops at the end of compute_grand_product (:472-504). Shares are tuples of `ncomp` integers on the `Ops` class of
tests/plonk_quot_ref.py. Also what the CPU and the GPU tests share: the plain chains around the four entries, the two closed permutation
instances, the closed lookup instance, and one random case of the four entries."""
import functools

from tests.plonk_rounds_ref import Ops, flat  # noqa: F401


# ---- active ranges (ActiveRegionData) -------------------------------------------------------------------------------------------------------
def active_idxs(ranges):
    return [i for s, e in ranges for i in range(s, e)]


def get_idx_fn(ranges):
    """-> (has_active_ranges, get_idx, active_domain_size or None)"""
    if ranges:
        idxs = active_idxs(ranges)
        return True, (lambda t: idxs[t]), len(idxs)
    return False, (lambda t: t), None


def promote_to_trivial_share(T, v):
    return T.add_with_public(T.default(), v)


# ---- 1. :98-160 ------------------------------------------------------------------------------------------------------------------------
def w4_records(T, w_l, w_r, w_o, w4, etas, read, write, shared):
    """shared: [(gate_idx, type_share)]. -> the new w_4 (the clone + resize of :133-137 is the caller's)"""
    out = list(w4)

    def inner(g):
        t = out[g]
        t = T.add(t, T.mul_with_public(w_l[g], etas[0]))
        t = T.add(t, T.mul_with_public(w_r[g], etas[1]))
        t = T.add(t, T.mul_with_public(w_o[g], etas[2]))
        out[g] = t

    for g in read:
        inner(g)
    for g in write:
        inner(g)
        out[g] = T.add_with_public(out[g], 1)
    for g, type_share in shared:
        inner(g)
        out[g] = T.add(type_share, out[g])
    return out


# ---- 2. :162-293 -------------------------------------------------------------------------------------------------------------------------
def shifted(T, w):
    """Polynomial::shifted as the loops read it: w[i + 1], and the default share behind the last row"""
    return list(w[1:]) + [T.default()]


def lookup_operands(T, w_l, w_r, w_o, tags, q_r, q_m, q_c, q_o, tables, q_lookup, beta, gamma):
    """-> (prod, sel): what :276 stores in lookup_inverses and q_lookup_mul_read_tag of :265-271"""
    p, n = T.p, len(w_l)
    b2, b3 = beta * beta % p, beta * beta % p * beta % p
    s_l, s_r, s_o = shifted(T, w_l), shifted(T, w_r), shifted(T, w_o)
    prod, sel = [], []
    for i in range(n):
        sel.append(T.add_with_public(T.mul_with_public(tags[i], (1 - q_lookup[i]) % p), q_lookup[i]))
        d1 = T.add(w_l[i], T.add_with_public(T.mul_with_public(s_l[i], q_r[i]), gamma))
        d2 = T.add(w_r[i], T.mul_with_public(s_r[i], q_m[i]))
        d3 = T.add(w_o[i], T.mul_with_public(s_o[i], q_c[i]))
        res = T.add(T.add(d1, T.mul_with_public(d2, beta)), T.mul_with_public(d3, b2))
        read = T.add_with_public(res, b3 * q_o[i] % p)
        write = (tables[0][i] + gamma + tables[1][i] * beta + tables[2][i] * b2 + tables[3][i] * b3) % p
        prod.append(T.mul_with_public(read, write))
    return prod, sel


# ---- 3. :344-451 ------------------------------------------------------------------------------------------------------------------------
def perm_operands(T, w, ident, sigma, beta, gamma, domain_size, ranges):
    """w = w_l, w_r, w_o, w_4. -> [n_1..n_4, d_1..d_4], active_domain_size - 1 shares each"""
    p = T.p
    has, get_idx, act = get_idx_fn(ranges)
    m = (act if has else domain_size) - 1
    out = [[] for _ in range(8)]
    for t in range(m):
        j = get_idx(t)
        for k in range(4):
            out[k].append(T.add_with_public(w[k][j], (ident[k][j] * beta + gamma) % p))
            out[4 + k].append(T.add_with_public(w[k][j], (sigma[k][j] * beta + gamma) % p))
    return out


# ---- 4. :472-504 ------------------------------------------------------------------------------------------------------------------------
def z_perm_place(T, mul, n, domain_size, ranges):
    has, get_idx, _ = get_idx_fn(ranges)
    z = [T.default()] * n
    z[1] = promote_to_trivial_share(T, 1)
    for i, v in enumerate(mul):
        z[get_idx(i + 1) if has else i + 1] = v
    if has:
        for i in range(domain_size):
            for j in range(len(ranges) - 1):
                if ranges[j][1] <= i < ranges[j + 1][0]:
                    z[i] = z[ranges[j + 1][0]]
                    break
    return z


# ---- the plain chains around the entries -------------------------------------------------------------------------------------------------
def grand_product_plain(p, n, w, ident, sigma, beta, gamma, domain_size, ranges):
    """compute_grand_product for one party that holds the values: -> (the 8 operand vectors, z_perm), integers"""
    T = Ops(p, 0, 0)
    sh = lambda v: [(x,) for x in v]
    ops = perm_operands(T, [sh(v) for v in w], ident, sigma, beta, gamma, domain_size, ranges)
    m = len(ops[0])
    num = [ops[0][t][0] * ops[1][t][0] % p * ops[2][t][0] % p * ops[3][t][0] % p for t in range(m)]
    den = [ops[4][t][0] * ops[5][t][0] % p * ops[6][t][0] % p * ops[7][t][0] % p for t in range(m)]
    for t in range(1, m):
        num[t] = num[t] * num[t - 1] % p
        den[t] = den[t] * den[t - 1] % p
    mul = [(num[t] * pow(den[t], -1, p) % p,) for t in range(m)]
    return [[x[0] for x in v] for v in ops], [x[0] for x in z_perm_place(T, mul, n, domain_size, ranges)]


def lookup_inverses_plain(p, w_l, w_r, w_o, tags, q_r, q_m, q_c, q_o, tables, q_lookup, beta, gamma):
    """compute_logderivative_inverses in the co-prover's selector form, for one party that holds the values: a zero stays zero.
    -> (prod, sel, inverses), integers"""
    T = Ops(p, 0, 0)
    sh = lambda v: [(x,) for x in v]
    prod, sel = lookup_operands(T, sh(w_l), sh(w_r), sh(w_o), sh(tags), q_r, q_m, q_c, q_o, tables, q_lookup, beta, gamma)
    x = [a[0] * b[0] % p for a, b in zip(prod, sel)]
    return [a[0] for a in prod], [b[0] for b in sel], [pow(v, -1, p) if v else 0 for v in x]


# ---- closed instances -------------------------------------------------------------------------------------------------------------------
RANGES_3 = [(0, 5), (8, 11), (14, 16)]


def perm_instance(p, r, n, rows):
    """rows: the active trace rows. The first and the last of them map to themselves (the last with free wires); random copy cycles of
    length 1, 2, 3 and 5 run over the cells of the rows between. -> (w, ident, sigma), 4 columns each"""
    w = [[0] * n for _ in range(4)]
    ident = [[k * n + i for i in range(n)] for k in range(4)]
    sigma = [row[:] for row in ident]
    cells = [(k, i) for k in range(4) for i in rows[1:-1]]
    r.shuffle(cells)
    pos = 0
    while pos < len(cells):
        ln = min(len(cells) - pos, r.choice([1, 2, 3, 5]))
        cyc = cells[pos:pos + ln]
        pos += ln
        v = r.randrange(p)
        for t, (k, i) in enumerate(cyc):
            w[k][i] = v
            k2, i2 = cyc[(t + 1) % ln]
            sigma[k][i] = ident[k2][i2]
    for k in range(4):
        w[k][rows[-1]] = r.randrange(p)
    return w, ident, sigma


def row_product(p, w, t, beta, gamma, i):
    return functools.reduce(lambda a, k: a * (w[k][i] + beta * t[k][i] + gamma) % p, range(4), 1)


def check_perm_closed_form(p, z, w, ident, sigma, beta, gamma, rows, n, ranges):
    """what a satisfied permutation leaves, for any challenges; rows = the active rows"""
    assert z[0] == 0 and z[1] == 1 and z[rows[-1]] == 1
    for a, b in zip(rows[1:-1], rows[2:]):
        assert z[b] * row_product(p, w, sigma, beta, gamma, a) % p == z[a] * row_product(p, w, ident, beta, gamma, a) % p, (a, b)
    if ranges:
        for (_, e), (s, _) in zip(ranges, ranges[1:]):
            assert all(z[i] == z[s] for i in range(e, s)), (e, s)
    else:
        assert all(v == 0 for v in z[rows[-1] + 1:])
    assert len(set(z[rows[1]:rows[-1] + 1])) > len(rows) // 2   # not a trivial product


@functools.lru_cache(maxsize=None)
def perm_closed(p, with_ranges):
    """n = 16: domain_size 13 without ranges, the ranges [0,5) [8,11) [14,16) with domain_size 16"""
    import random
    r = random.Random(7 + with_ranges)
    n = 16
    ranges = RANGES_3 if with_ranges else None
    rows = active_idxs(ranges) if with_ranges else list(range(13))
    domain_size = 16 if with_ranges else 13
    w, ident, sigma = perm_instance(p, r, n, rows)
    beta, gamma = r.randrange(1, p), r.randrange(1, p)
    ops, z = grand_product_plain(p, n, w, ident, sigma, beta, gamma, domain_size, ranges)
    return dict(n=n, ranges=ranges, rows=rows, domain_size=domain_size, w=w, ident=ident, sigma=sigma, beta=beta, gamma=gamma, ops=ops, z=z)


@functools.lru_cache(maxsize=None)
def lookup_closed(p):
    """n = 16, five table rows, six lookup gates at rows 7, 8, 9, 11, 13 and 15 (row 15: the shifted wire is zero) with random non-zero step
    sizes, filled from the highest row down so that each shifted value is final when it is read"""
    import random
    r = random.Random(11)
    n, trow, gates = 16, list(range(2, 7)), [7, 8, 9, 11, 13, 15]
    tables = [[r.randrange(p) for _ in range(n)] for _ in range(4)]
    w_l, w_r, w_o = ([r.randrange(p) for _ in range(n)] for _ in range(3))
    q_o = [r.randrange(p) for _ in range(n)]
    q_r, q_m, q_c = ([r.randrange(1, p) for _ in range(n)] for _ in range(3))
    q_lookup, counts = [0] * n, [0] * n
    for g in reversed(gates):
        t = r.choice(trow[:3])
        counts[t] += 1
        q_lookup[g] = 1
        s = lambda v: v[g + 1] if g + 1 < n else 0
        w_l[g] = (tables[0][t] - q_r[g] * s(w_l)) % p
        w_r[g] = (tables[1][t] - q_m[g] * s(w_r)) % p
        w_o[g] = (tables[2][t] - q_c[g] * s(w_o)) % p
        q_o[g] = tables[3][t]
    tags = [1 if c else 0 for c in counts]
    beta, gamma = r.randrange(1, p), r.randrange(1, p)
    prod, sel, inv = lookup_inverses_plain(p, w_l, w_r, w_o, tags, q_r, q_m, q_c, q_o, tables, q_lookup, beta, gamma)
    return dict(n=n, w=[w_l, w_r, w_o], tags=tags, q=[q_r, q_m, q_c, q_o], tables=tables, q_lookup=q_lookup, counts=counts, beta=beta, gamma=gamma,
                prod=prod, sel=sel, inv=inv)


def check_lookup_closed_form(p, c):
    """I != 0 exactly where q_lookup or the tag is 1, and sum q_lookup I write - count I read = 0"""
    n, inv = c["n"], c["inv"]
    assert all((inv[i] != 0) == bool(c["q_lookup"][i] or c["tags"][i]) for i in range(n))
    # the read and the write term alone, from their definitions (the entries give only their product)
    b, g = c["beta"], c["gamma"]
    b2, b3 = b * b % p, b * b * b % p
    w_l, w_r, w_o = c["w"]
    q_r, q_m, q_c, q_o = c["q"]
    s = lambda v, i: v[i + 1] if i + 1 < n else 0
    total = 0
    for i in range(n):
        read = (w_l[i] + g + q_r[i] * s(w_l, i) + b * (w_r[i] + q_m[i] * s(w_r, i)) + b2 * (w_o[i] + q_c[i] * s(w_o, i)) + b3 * q_o[i]) % p
        write = (c["tables"][0][i] + g + c["tables"][1][i] * b + c["tables"][2][i] * b2 + c["tables"][3][i] * b3) % p
        assert read * write % p == c["prod"][i], i
        total += c["q_lookup"][i] * inv[i] * write - c["counts"][i] * inv[i] * read
    assert total % p == 0


# ---- one case of the four entries ------------------------------------------------------------------------------------------------------
def entries_case(p, T, n, draw, domain_size, ranges, records=None, bits=None):
    """inputs of the four entries and what the restatement makes of them. draw(): one field element; bits(): the value of a selector or
    tag entry (default: draw). records = (read, write, shared rows); default: a few rows with 0 and n - 1 among them."""
    sh = lambda: tuple(draw() for _ in range(T.ncomp))
    vec = lambda k: [sh() for _ in range(k)]
    pub = lambda k: [draw() for _ in range(k)]
    bits = bits or draw
    c = {"n": n, "domain_size": domain_size, "ranges": ranges}
    c["w"] = [vec(n) for _ in range(4)]
    c["etas"] = pub(3)
    if records is None:
        rows = list(range(n))
        records = ([0, 5 % n, 7 % n][:min(3, n // 4)], [n - 1, 2], [3, 9 % n])
        assert len(set(sum(records, []))) == len(sum(records, [])) and all(x in rows for x in sum(records, []))
    c["records"] = records
    c["type_share"] = vec(len(records[2]))
    c["want_w4"] = w4_records(T, c["w"][0], c["w"][1], c["w"][2], c["w"][3], c["etas"], records[0], records[1], list(zip(records[2], c["type_share"])))
    c["tags"] = [tuple(bits() for _ in range(T.ncomp)) for _ in range(n)]
    c["q"] = [pub(n) for _ in range(4)]
    c["tables"] = [pub(n) for _ in range(4)]
    c["q_lookup"] = [bits() for _ in range(n)]
    c["ch"] = pub(2)
    c["want_lookup"] = lookup_operands(T, c["w"][0], c["w"][1], c["w"][2], c["tags"], *c["q"], c["tables"], c["q_lookup"], *c["ch"])
    c["ident"] = [pub(n) for _ in range(4)]
    c["sigma"] = [pub(n) for _ in range(4)]
    c["want_perm"] = perm_operands(T, c["w"], c["ident"], c["sigma"], *c["ch"], domain_size, ranges)
    m = len(c["want_perm"][0])
    c["mul"] = vec(m)
    c["want_z"] = z_perm_place(T, c["mul"], n, domain_size, ranges)
    return c
