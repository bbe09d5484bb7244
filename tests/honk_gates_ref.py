"""The other five relations of co-noir's UltraHonk sumcheck round, restated in Python integers from the PROVER side of the reference: the
`accumulate` bodies over univariates of length 7 of EllipticRelation (relations/elliptic_relation.rs:81-161), MemoryRelation
(memory_relation.rs:145-358), NonNativeFieldRelation (non_native_field_relation.rs:85-177), Poseidon2ExternalRelation
(poseidon2_external_relation.rs:121-205) and Poseidon2InternalRelation (poseidon2_internal_relation.rs:118-200), truncated to the
accumulator lengths, with the five skips, inside the loop of SumcheckProverRound::compute_univariate_inner
(sumcheck_round_prover.rs:224-255); and batch_over_relations_univariates over all 28 accumulators (:76-122, relations/mod.rs:134-199).
Univariates, extension, the gate separator and the first eleven subrelations are tests/honk_relations_ref.py's, imported and not
edited. The device's per-point functions are written from the scalar verify_accumulate bodies; `relations_at_point` restates those
too. Also what the CPU and the GPU tests share: a satisfied trace in closed form with every gate kind, and a random case with planted
skip edges."""
import functools
import random

from oracle import curves as CV
from tests import honk_relations_ref as R

Uni = R.Uni
MAX_PARTIAL_RELATION_LENGTH = R.MAX_PARTIAL_RELATION_LENGTH
WITNESS = ["w_l", "w_r", "w_o", "w_4"]
SHIFTED = ["w_l_shift", "w_r_shift", "w_o_shift", "w_4_shift"]
PRECOMPUTED = ["q_m", "q_c", "q_l", "q_r", "q_o", "q_4"]
SELECTORS = ["q_elliptic", "q_memory", "q_nnf", "q_poseidon2_external", "q_poseidon2_internal"]
COLS = WITNESS + SHIFTED + PRECOMPUTED + SELECTORS          # the order of cols_dev
PARAMS = ["eta_1", "eta_2", "eta_3", "curve_b", "diag_0", "diag_1", "diag_2", "diag_3"]
RELATIONS = ["elliptic", "memory", "nnf", "poseidon2_external", "poseidon2_internal"]
SELECTOR_OF = dict(zip(RELATIONS, SELECTORS))
SUBRELATIONS = (["elliptic.r0", "elliptic.r1"] + ["memory.r%d" % i for i in range(6)] + ["nnf.r0"] +
                ["poseidon2_external.r%d" % i for i in range(4)] + ["poseidon2_internal.r%d" % i for i in range(4)])
ACC_LEN = [6] * 9 + [7] * 8                                 # the reference's accumulator lengths
RELATION_OF = {"elliptic": [0, 1], "memory": [2, 3, 4, 5, 6, 7], "nnf": [8], "poseidon2_external": [9, 10, 11, 12],
               "poseidon2_internal": [13, 14, 15, 16]}
ALL_COLS = R.COLS + SELECTORS                               # the 41 distinct columns of the two entries
ALL_ACC_LEN = R.ACC_LEN + ACC_LEN
ALL_SUBRELATIONS = R.SUBRELATIONS + SUBRELATIONS
NUM_ALPHAS = 27
LIMB_SIZE, SUBLIMB_SHIFT = 1 << 68, 1 << 14
assert len(COLS) == 19 and len(SUBRELATIONS) == 17 and sum(ACC_LEN) == 110 and len(ALL_COLS) == 41 and len(ALL_ACC_LEN) == 28


def extend_edges(p, polys, edge_idx):
    return {c: Uni(p, R.extend_from(p, [polys[c][edge_idx], polys[c][edge_idx + 1]], MAX_PARTIAL_RELATION_LENGTH)) for c in COLS}


def skip(relation, e):
    """Relation::skip of the five files: the selector's univariate is zero"""
    return e[SELECTOR_OF[relation]].is_zero()


# ---- accumulate, prover side: -> the univariates (length 7) that are added to r0, r1, ... ------------------------------------------------
def accumulate_elliptic(p, e, params, sf):
    x_1, y_1 = e["w_r"], e["w_o"]
    x_2, y_2, y_3, x_3 = e["w_l_shift"], e["w_4_shift"], e["w_o_shift"], e["w_r_shift"]
    q_sign, q_elliptic, q_is_double = e["q_l"], e["q_elliptic"], e["q_m"]
    x_diff = x_2 - x_1
    y2_sqr, y1_sqr = y_2.sqr(), y_1.sqr()
    y1y2 = y_1 * y_2 * q_sign
    x_add_identity = (x_3 + x_2 + x_1) * x_diff.sqr() - y2_sqr - y1_sqr + y1y2 + y1y2
    q_elliptic_by_scaling = q_elliptic * sf
    q_elliptic_q_double_scaling = q_elliptic_by_scaling * q_is_double
    q_elliptic_not_double_scaling = q_elliptic_by_scaling - q_elliptic_q_double_scaling
    tmp_1 = x_add_identity * q_elliptic_not_double_scaling
    y1_plus_y3 = y_1 + y_3
    y_diff = y_2 * q_sign - y_1
    y_add_identity = y1_plus_y3 * x_diff + (x_3 - x_1) * y_diff
    tmp_2 = y_add_identity * q_elliptic_not_double_scaling
    curve_b = params[3]
    x1_mul_3 = x_1 + x_1 + x_1
    x_pow_4_mul_3 = (y1_sqr - curve_b) * x1_mul_3
    y1_sqr_mul_4 = y1_sqr + y1_sqr
    y1_sqr_mul_4 = y1_sqr_mul_4 + y1_sqr_mul_4
    x1_pow_4_mul_9 = x_pow_4_mul_3 + x_pow_4_mul_3 + x_pow_4_mul_3
    x_double_identity = (x_3 + x_1 + x_1) * y1_sqr_mul_4 - x1_pow_4_mul_9
    tmp_1 = tmp_1 + x_double_identity * q_elliptic_q_double_scaling
    x1_sqr_mul_3 = x1_mul_3 * x_1
    y_double_identity = x1_sqr_mul_3 * (x_1 - x_3) - (y_1 + y_1) * y1_plus_y3
    tmp_2 = tmp_2 + y_double_identity * q_elliptic_q_double_scaling
    return [tmp_1, tmp_2]


def accumulate_memory(p, e, params, sf):
    eta, eta_two, eta_three = params[0], params[1], params[2]
    w_1, w_2, w_3, w_4 = e["w_l"], e["w_r"], e["w_o"], e["w_4"]
    w_1_shift, w_2_shift, w_3_shift, w_4_shift = e["w_l_shift"], e["w_r_shift"], e["w_o_shift"], e["w_4_shift"]
    q_1, q_2, q_3, q_4, q_m, q_c, q_memory = e["q_l"], e["q_r"], e["q_o"], e["q_4"], e["q_m"], e["q_c"], e["q_memory"]
    memory_record_check = w_3 * eta_three
    memory_record_check = memory_record_check + w_2 * eta_two
    memory_record_check = memory_record_check + w_1 * eta
    memory_record_check = memory_record_check + q_c
    partial_record_check = memory_record_check
    memory_record_check = memory_record_check - w_4
    neg_index_delta = w_1 - w_1_shift
    index_delta_is_zero = neg_index_delta + 1
    record_delta = w_4_shift - w_4
    index_is_monotonically_increasing = neg_index_delta.sqr() + neg_index_delta
    adjacent_values_match_if_adjacent_indices_match = index_delta_is_zero * record_delta
    q_memory_by_scaling = q_memory * sf
    q_one_by_two = q_1 * q_2
    q_one_by_two_by_memory_by_scaling = q_one_by_two * q_memory_by_scaling
    r1 = adjacent_values_match_if_adjacent_indices_match * q_one_by_two_by_memory_by_scaling
    r2 = index_is_monotonically_increasing * q_one_by_two_by_memory_by_scaling
    rom_consistency_check_identity = memory_record_check * q_one_by_two
    neg_access_type = partial_record_check - w_4
    access_check = neg_access_type.sqr() + neg_access_type
    neg_next_gate_access_type = w_3_shift * eta_three
    neg_next_gate_access_type = neg_next_gate_access_type + w_2_shift * eta_two
    neg_next_gate_access_type = neg_next_gate_access_type + w_1_shift * eta
    neg_next_gate_access_type = neg_next_gate_access_type - w_4_shift
    value_delta = w_3_shift - w_3
    adjacent_values_match_and_next_is_a_read = (index_delta_is_zero * value_delta) * (neg_next_gate_access_type + 1)
    next_gate_access_type_is_boolean = neg_next_gate_access_type.sqr() + neg_next_gate_access_type
    q_3_by_memory_and_scaling = q_3 * q_memory_by_scaling
    r3 = adjacent_values_match_and_next_is_a_read * q_3_by_memory_and_scaling
    r4 = index_is_monotonically_increasing * q_3_by_memory_and_scaling
    r5 = next_gate_access_type_is_boolean * q_3_by_memory_and_scaling
    ram_consistency_check_identity = access_check * q_3_by_memory_and_scaling
    timestamp_delta = w_2_shift - w_2
    ram_timestamp_check_identity = index_delta_is_zero * timestamp_delta - w_3
    memory_identity = rom_consistency_check_identity
    memory_identity = memory_identity + ram_timestamp_check_identity * (q_4 * q_1)
    memory_identity = memory_identity + memory_record_check * (q_m * q_1)
    memory_identity = memory_identity * q_memory_by_scaling          # memory_relation.rs:352: before the RAM term is added
    memory_identity = memory_identity + ram_consistency_check_identity
    return [memory_identity, r1, r2, r3, r4, r5]


def accumulate_nnf(p, e, params, sf):
    w_1, w_2, w_3, w_4 = e["w_l"], e["w_r"], e["w_o"], e["w_4"]
    w_1_shift, w_2_shift, w_3_shift, w_4_shift = e["w_l_shift"], e["w_r_shift"], e["w_o_shift"], e["w_4_shift"]
    q_2, q_3, q_4, q_m, q_nnf = e["q_r"], e["q_o"], e["q_4"], e["q_m"], e["q_nnf"]
    limb_size, sublimb_shift = LIMB_SIZE % p, SUBLIMB_SHIFT % p
    limb_subproduct = w_1 * w_2_shift + w_1_shift * w_2
    non_native_field_gate_2 = w_1 * w_4 + w_2 * w_3 - w_3_shift
    non_native_field_gate_2 = non_native_field_gate_2 * limb_size
    non_native_field_gate_2 = non_native_field_gate_2 - w_4_shift
    non_native_field_gate_2 = non_native_field_gate_2 + limb_subproduct
    non_native_field_gate_2 = non_native_field_gate_2 * q_4
    limb_subproduct = limb_subproduct * limb_size
    limb_subproduct = limb_subproduct + w_1_shift * w_2_shift
    non_native_field_gate_1 = limb_subproduct - (w_3 + w_4)
    non_native_field_gate_1 = non_native_field_gate_1 * q_3
    non_native_field_gate_3 = limb_subproduct + w_4
    non_native_field_gate_3 = non_native_field_gate_3 - (w_3_shift + w_4_shift)
    non_native_field_gate_3 = non_native_field_gate_3 * q_m
    non_native_field_identity = (non_native_field_gate_1 + non_native_field_gate_2 + non_native_field_gate_3) * q_2
    limb_accumulator_1 = w_2_shift * sublimb_shift
    for t in (w_1_shift, w_3, w_2):
        limb_accumulator_1 = (limb_accumulator_1 + t) * sublimb_shift
    limb_accumulator_1 = (limb_accumulator_1 + w_1 - w_4) * q_4
    limb_accumulator_2 = w_3_shift * sublimb_shift
    for t in (w_2_shift, w_1_shift, w_4):
        limb_accumulator_2 = (limb_accumulator_2 + t) * sublimb_shift
    limb_accumulator_2 = (limb_accumulator_2 + w_3 - w_4_shift) * q_m
    limb_accumulator_identity = (limb_accumulator_1 + limb_accumulator_2) * q_3
    return [(non_native_field_identity + limb_accumulator_identity) * q_nnf * sf]


def _sbox(s):
    return s.sqr().sqr() * s


def accumulate_poseidon2_external(p, e, params, sf):
    u1, u2 = _sbox(e["w_l"] + e["q_l"]), _sbox(e["w_r"] + e["q_r"])
    u3, u4 = _sbox(e["w_o"] + e["q_o"]), _sbox(e["w_4"] + e["q_4"])
    t0 = u1 + u2
    t1 = u3 + u4
    t2 = u2 + u2 + t1
    t3 = u4 + u4 + t0
    v4 = t1 + t1
    v4 = v4 + v4 + t3
    v2 = t0 + t0
    v2 = v2 + v2 + t2
    v1 = t3 + v2
    v3 = t2 + v4
    q_pos_by_scaling = e["q_poseidon2_external"] * sf
    return [(v - e[w]) * q_pos_by_scaling for v, w in zip((v1, v2, v3, v4), SHIFTED)]


def accumulate_poseidon2_internal(p, e, params, sf):
    u = [_sbox(e["w_l"] + e["q_l"]), e["w_r"], e["w_o"], e["w_4"]]
    total = u[0] + u[1] + u[2] + u[3]
    q_pos_by_scaling = e["q_poseidon2_internal"] * sf
    return [(u[i] * params[4 + i] + total - e[SHIFTED[i]]) * q_pos_by_scaling for i in range(4)]


ACCUMULATE = {"elliptic": accumulate_elliptic, "memory": accumulate_memory, "nnf": accumulate_nnf,
              "poseidon2_external": accumulate_poseidon2_external, "poseidon2_internal": accumulate_poseidon2_internal}


def edge_contribution(p, polys, edge_idx, params, sf, relation, honour_skip=True, eager_skip=False):
    """what one edge adds to the relation's accumulators (truncated to their lengths); all zeros when the edge is skipped. eager_skip: the
    WRONG skip that fires on zero at the first end alone -- what the planted one-end edges are there to tell apart."""
    e = extend_edges(p, polys, edge_idx)
    idx = RELATION_OF[relation]
    if (honour_skip and skip(relation, e)) or (eager_skip and polys[SELECTOR_OF[relation]][edge_idx] == 0):
        return [[0] * ACC_LEN[s] for s in idx]
    return [u.ev[:ACC_LEN[s]] for s, u in zip(idx, ACCUMULATE[relation](p, e, params, sf))]


def accumulate_range(p, polys, edge_begin, edge_end, scaling, stride, params, honour_skip=True, eager_skip=False):
    """the loop of compute_univariate_inner over (edge_begin..edge_end).step_by(2) -> the seventeen accumulators"""
    acc = [[0] * ln for ln in ACC_LEN]
    for edge_idx in range(edge_begin, edge_end, 2):
        sf = R.scaling_of(p, edge_idx, scaling, stride)
        for relation in RELATIONS:
            for s, c in zip(RELATION_OF[relation], edge_contribution(p, polys, edge_idx, params, sf, relation, honour_skip, eager_skip)):
                acc[s] = [(a + b) % p for a, b in zip(acc[s], c)]
    return acc


def split_acc(flat):
    acc, at = [], 0
    for ln in ACC_LEN:
        acc.append(list(flat[at:at + ln]))
        at += ln
    assert at == len(flat)
    return acc


# ---- the scalar shape (verify_accumulate), for the comparison of the two shapes -----------------------------------------------------------
def relations_at_point(p, v, params, sf):
    """v: column name -> value at one point. -> the seventeen subrelation values"""
    eta, eta2, eta3, b = params[:4]
    w1, w2, w3, w4 = (v[c] for c in WITNESS)
    w1s, w2s, w3s, w4s = (v[c] for c in SHIFTED)
    qm, qc, q1, q2, q3, q4 = (v[c] for c in PRECOMPUTED)
    # elliptic: x_1 = w_r, y_1 = w_o, x_2 = w_l', y_2 = w_4', x_3 = w_r', y_3 = w_o', q_sign = q_l, q_is_double = q_m
    x1, y1, x2, y2, x3, y3 = w2, w3, w1s, w4s, w2s, w3s
    qe = v["q_elliptic"] * sf
    x_add = (x3 + x2 + x1) * (x2 - x1) ** 2 - y2 * y2 - y1 * y1 + 2 * y1 * y2 * q1
    y_add = (y1 + y3) * (x2 - x1) + (x3 - x1) * (y2 * q1 - y1)
    x_dbl = (x3 + 2 * x1) * 4 * y1 * y1 - 9 * (y1 * y1 - b) * x1
    y_dbl = 3 * x1 * x1 * (x1 - x3) - 2 * y1 * (y1 + y3)
    out = [(x_add * (1 - qm) + x_dbl * qm) * qe, (y_add * (1 - qm) + y_dbl * qm) * qe]
    # memory
    record = qc + w1 * eta + w2 * eta2 + w3 * eta3 - w4
    nid = w1 - w1s
    mono = nid * nid + nid
    qms = v["q_memory"] * sf
    nxt = w1s * eta + w2s * eta2 + w3s * eta3 - w4s
    ident = record * q1 * q2 + ((nid + 1) * (w2s - w2) - w3) * q4 * q1 + record * qm * q1
    out += [ident * qms + (record * record + record) * q3 * qms, (nid + 1) * (w4s - w4) * q1 * q2 * qms, mono * q1 * q2 * qms,
            (nid + 1) * (w3s - w3) * (nxt + 1) * q3 * qms, mono * q3 * qms, (nxt * nxt + nxt) * q3 * qms]
    # nnf
    L, S = LIMB_SIZE, SUBLIMB_SHIFT
    lo = w1 * w2s + w1s * w2
    hi = lo * L + w1s * w2s
    g1 = (hi - w3 - w4) * q3
    g2 = ((w1 * w4 + w2 * w3 - w3s) * L - w4s + lo) * q4
    g3 = (hi + w4 - w3s - w4s) * qm
    la1 = ((((w2s * S + w1s) * S + w3) * S + w2) * S + w1 - w4) * q4
    la2 = ((((w3s * S + w2s) * S + w1s) * S + w4) * S + w3 - w4s) * qm
    out.append(((g1 + g2 + g3) * q2 + (la1 + la2) * q3) * v["q_nnf"] * sf)
    # Poseidon2: the external matrix by its rows (5 7 1 3), (4 6 1 1), (1 3 5 7), (1 1 4 6)
    u = [pow(w + q, 5, p) for w, q in ((w1, q1), (w2, q2), (w3, q3), (w4, q4))]
    qs = v["q_poseidon2_external"] * sf
    for row, ws in zip(((5, 7, 1, 3), (4, 6, 1, 1), (1, 3, 5, 7), (1, 1, 4, 6)), (w1s, w2s, w3s, w4s)):
        out.append((sum(c * x for c, x in zip(row, u)) - ws) * qs)
    ui = [u[0], w2, w3, w4]
    qs = v["q_poseidon2_internal"] * sf
    for i, ws in enumerate((w1s, w2s, w3s, w4s)):
        out.append((ui[i] * params[4 + i] + sum(ui) - ws) * qs)
    return [x % p for x in out]


# ---- batching over all 28 accumulators ----------------------------------------------------------------------------------------------------
def batch_over_relations_univariates_all(p, acc, alphas, current_element, partial_evaluation_result, size=R.BATCHED_RELATION_PARTIAL_LENGTH):
    """AllRelationAcc::scale with first_scalar = 1 and alphas[0..27) in the order arith, perm, lookup, delta, elliptic, memory, nnf,
    poseidon2_external, poseidon2_internal, then extend_and_batch_univariates: every subrelation but lookup.r1 is linearly independent and
    takes the [1, beta_i] factor and partial_evaluation_result"""
    assert len(acc) == 28 and len(alphas) == NUM_ALPHAS and [len(a) for a in acc] == ALL_ACC_LEN
    scalars = [1] + list(alphas)
    extended_random = R.extend_from(p, [1, current_element], size)
    result = [0] * size
    for s, a in enumerate(acc):
        ext = R.extend_from(p, [v * scalars[s] % p for v in a], size)
        for i in range(size):
            if s == R.LINEARLY_DEPENDENT:
                result[i] = (result[i] + ext[i]) % p
            else:
                result[i] = (result[i] + ext[i] * extended_random[i] % p * partial_evaluation_result) % p
    return result


def check_round_chain_all(p, n, betas, alphas, challenges, accumulators_of_round, fold_all):
    """The sumcheck identities of a satisfied trace over log2(n) rounds on all 28 accumulators. accumulators_of_round(round, size,
    gate_separator) -> the 28 accumulators of the current columns; fold_all(u) folds every column. Asserts: in round 0 entries 0 and 1 of
    every accumulator but lookup.r1 are zero; S(0) + S(1) = 0 in round 0; S'(0) + S'(1) = S(u) afterwards; the tail of S is not zero."""
    log_n = n.bit_length() - 1
    gs = R.GateSeparator(p, betas, log_n)
    target, size = 0, n
    for rnd in range(log_n):
        acc = accumulators_of_round(rnd, size, gs)
        if rnd == 0:
            for s, a in enumerate(acc):
                if s == R.LINEARLY_DEPENDENT:
                    assert (a[0] + a[1]) % p == 0 and a[0] != 0
                else:
                    assert a[0] == 0 and a[1] == 0, (ALL_SUBRELATIONS[s], "vanishes on every row of a satisfied trace")
        S = batch_over_relations_univariates_all(p, acc, alphas, gs.current_element(), gs.partial_evaluation_result)
        assert (S[0] + S[1]) % p == target, ("round", rnd)
        assert any(S[2:]), "the round univariate is not trivially zero"
        u = challenges[rnd]
        target = R.lagrange_eval(p, S, u)
        gs.partially_evaluate(u)
        fold_all(u)
        size >>= 1
    return target


# ---- a satisfied trace in closed form ----------------------------------------------------------------------------------------------------------
GATE_KINDS = ["elliptic.add", "elliptic.sub", "elliptic.double", "poseidon2_external", "poseidon2_internal", "memory.record", "memory.rom",
              "memory.rom_next_index", "memory.ram", "memory.ram_next_index", "memory.timestamp", "nnf.gate_1", "nnf.gate_2", "nnf.gate_3",
              "nnf.limb_accumulator_1", "nnf.limb_accumulator_2"]
FIRST_GATE_ROW = 16


def _curve_points(p, r):
    """-> curve_b and two points P_1, P_2 (x_1 != x_2) of y^2 = x^3 + curve_b over the field of p elements: multiples of the generator of
    Grumpkin, y^2 = x^3 - 17, over BN254 Fr; elsewhere the curve through a random point, and that point and its double."""
    G = CV.GRUMPKIN_G1
    if G.F.p == p:
        pt = lambda k: functools.reduce(lambda acc, _: G.add(acc, G.gen), range(k - 1), G.gen)
        P1, P2 = pt(r.randrange(2, 40)), pt(r.randrange(41, 80))
        assert G.is_on_curve(P1) and G.is_on_curve(P2)
        return G.b % p, P1, P2
    x, y = r.randrange(1, p), r.randrange(1, p)
    b = (y * y - x * x * x) % p
    lam = 3 * x * x * pow(2 * y, -1, p) % p
    x2 = (lam * lam - 2 * x) % p
    return b, (x, y), (x2, (lam * (x - x2) - y) % p)


@functools.lru_cache(maxsize=None)
def satisfied_trace(p):
    """The 16-row trace of tests/honk_relations_ref.py in rows 0 .. 15 of n = 64 (its relations see nothing behind their last row: their
    selectors, z_perm and the inverses are zero there), and from row 16 on one gate of each kind of GATE_KINDS at every other row, each
    followed by a row without selectors that leaves its shifted wires free. Every identity is linear in one wire of the gate's row or of
    the next, which is solved for; all other wires and the selectors that are on are random, so the trace is satisfied for any etas and
    any diagonal values. -> dict(n, polys (the 41 columns), params (beta, gamma, public_input_delta), gate_params (the eight), rows)"""
    base = R.satisfied_trace(p)
    r = random.Random(4242)
    n, n0 = 64, base["n"]
    rnd = lambda: r.randrange(1, p)
    inv = lambda x: pow(x % p, -1, p)
    gate_params = [rnd() for _ in range(8)]
    eta, eta2, eta3 = gate_params[:3]
    curve_b, P1, P2 = _curve_points(p, r)
    gate_params[3] = curve_b
    diag = gate_params[4:]
    L, S = LIMB_SIZE % p, SUBLIMB_SHIFT % p
    polys = {c: list(base["polys"][c]) + [0] * (n - n0) for c in R.COLS if not c.endswith("_shift")}
    for k in range(4):
        for i in range(n0, n):
            polys["sigma_%d" % (k + 1)][i] = polys["id_%d" % (k + 1)][i] = k * n + i
    for c in SELECTORS:
        polys[c] = [0] * n
    w = [polys[c] for c in WITNESS]
    for i in range(n0, n):
        for k in range(4):
            w[k][i] = rnd()
    rows = {}
    for t, kind in enumerate(GATE_KINDS):
        g = FIRST_GATE_ROW + 2 * t
        rows[kind] = g
        rel = kind.split(".")[0]
        polys[SELECTOR_OF[rel]][g] = rnd() if rel != "elliptic" else 1
        on = lambda *cs: [polys[c].__setitem__(g, rnd()) for c in cs]
        w1, w2, w3, w4 = (w[k][g] for k in range(4))
        w1s, w2s, w3s, w4s = (w[k][g + 1] for k in range(4))
        if kind in ("elliptic.add", "elliptic.sub"):
            s = 1 if kind == "elliptic.add" else p - 1
            polys["q_l"][g] = s
            (x1, y1), (x2, y2) = P1, P2
            x3 = ((y2 - s * y1) ** 2 * inv((x2 - x1) ** 2) - x2 - x1) % p
            y3 = (-y1 - (x3 - x1) * (y2 * s - y1) * inv(x2 - x1)) % p
            if CV.GRUMPKIN_G1.F.p == p:     # the gate computes P_2 + P_1 and, with q_sign = -1, P_1 - P_2
                G = CV.GRUMPKIN_G1
                assert (x3, y3) == (G.add(P1, P2) if s == 1 else G.add(P1, G.neg(P2))), kind
            w[1][g], w[2][g], w[0][g + 1], w[3][g + 1], w[1][g + 1], w[2][g + 1] = x1, y1, x2, y2, x3, y3
        elif kind == "elliptic.double":
            polys["q_m"][g], polys["q_l"][g] = 1, rnd()
            x1, y1 = P2
            x3 = (9 * x1 * (y1 * y1 - curve_b) * inv(4 * y1 * y1) - 2 * x1) % p
            y3 = (3 * x1 * x1 * (x1 - x3) * inv(2 * y1) - y1) % p
            if CV.GRUMPKIN_G1.F.p == p:
                assert (x3, y3) == CV.GRUMPKIN_G1.double(P2)
            w[1][g], w[2][g], w[1][g + 1], w[2][g + 1] = x1, y1, x3, y3
        elif kind == "poseidon2_external":
            on("q_l", "q_r", "q_o", "q_4")
            u = [pow(w[k][g] + polys[c][g], 5, p) for k, c in enumerate(("q_l", "q_r", "q_o", "q_4"))]
            for k, row in enumerate(((5, 7, 1, 3), (4, 6, 1, 1), (1, 3, 5, 7), (1, 1, 4, 6))):
                w[k][g + 1] = sum(c * x for c, x in zip(row, u)) % p
        elif kind == "poseidon2_internal":
            on("q_l")
            u = [pow(w1 + polys["q_l"][g], 5, p), w2, w3, w4]
            for k in range(4):
                w[k][g + 1] = (u[k] * diag[k] + sum(u)) % p
        elif kind == "memory.record":          # q_m q_l: q_c + w_1 eta + w_2 eta_2 + w_3 eta_3 - w_4 = 0
            on("q_m", "q_l", "q_c")
            w[3][g] = (polys["q_c"][g] + w1 * eta + w2 * eta2 + w3 * eta3) % p
        elif kind in ("memory.rom", "memory.rom_next_index"):   # q_l q_r: the record, a monotone index, equal records at equal indices
            on("q_l", "q_r")
            w[3][g] = (w1 * eta + w2 * eta2 + w3 * eta3) % p
            if kind == "memory.rom":
                w[0][g + 1], w[3][g + 1] = w1, w[3][g]
            else:
                w[0][g + 1] = (w1 + 1) % p
        elif kind in ("memory.ram", "memory.ram_next_index"):   # q_o: boolean access types, a monotone index, a read returns the value
            on("q_o")
            w[3][g] = (w1 * eta + w2 * eta2 + w3 * eta3 + 1) % p                      # this access is a write
            if kind == "memory.ram":
                w[0][g + 1], w[2][g + 1] = w1, w3                                      # same index, the next access reads the value
                w[3][g + 1] = (w[0][g + 1] * eta + w2s * eta2 + w[2][g + 1] * eta3) % p
            else:
                w[0][g + 1] = (w1 + 1) % p                                             # next index, the next access writes
                w[3][g + 1] = (w[0][g + 1] * eta + w2s * eta2 + w3s * eta3 + 1) % p
        elif kind == "memory.timestamp":       # q_4 q_l: w_3 = (1 - index delta) (timestamp' - timestamp)
            on("q_4", "q_l")
            w[0][g + 1] = w1
            w[2][g] = (w2s - w2) % p
        else:
            lo = (w1 * w2s + w1s * w2) % p
            hi = (lo * L + w1s * w2s) % p
            if kind == "nnf.gate_1":
                on("q_r", "q_o")
                w[3][g] = (hi - w3) % p
            elif kind == "nnf.gate_2":
                on("q_r", "q_4")
                w[3][g + 1] = ((w1 * w4 + w2 * w3 - w3s) * L + lo) % p
            elif kind == "nnf.gate_3":
                on("q_r", "q_m")
                w[3][g] = (w3s + w4s - hi) % p
            elif kind == "nnf.limb_accumulator_1":
                on("q_o", "q_4")
                w[3][g] = (((((w2s * S + w1s) * S + w3) * S + w2) * S) + w1) % p
            else:
                on("q_o", "q_m")
                w[3][g + 1] = (((((w3s * S + w2s) * S + w1s) * S + w4) * S) + w3) % p
    shift = lambda v: v[1:] + [0]
    for c in ("w_l", "w_r", "w_o", "w_4", "z_perm"):
        polys[c + "_shift"] = shift(polys[c])
    assert set(polys) == set(ALL_COLS)
    return dict(n=n, polys=polys, params=base["params"], gate_params=tuple(gate_params), rows=rows)


# ---- a random case with planted skip edges ---------------------------------------------------------------------------------------------------
PLANTS = [rel + kind for rel in RELATIONS for kind in (".skip", ".one_end")]


def random_case(p, n, seed, plants=True):
    """n elements per column of random (unsatisfied) data, every term non-zero. Planted from the last edge down, edge 0 left alone: for each
    of the five selectors one edge where it is zero at both ends (left out; it would have added zeros) and one where it is zero at the
    first end only (counted). -> dict(polys, params (the eight), planted: name -> edge_idx)"""
    r = random.Random(seed)
    polys = {c: [r.randrange(1, p) for _ in range(n)] for c in COLS}
    params = tuple(r.randrange(1, p) for _ in range(8))
    planted = {}
    edges = n // 2
    for i, name in enumerate(PLANTS[:max(0, edges - 1)] if plants else []):
        e = 2 * (edges - 1 - i)
        rel, kind = name.split(".")
        for x in ((e, e + 1) if kind == "skip" else (e,)):
            polys[SELECTOR_OF[rel]][x] = 0
        planted[name] = e
    return dict(n=n, polys=polys, params=params, planted=planted)
