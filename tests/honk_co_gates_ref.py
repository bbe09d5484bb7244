"""The sumcheck round of co-noir's collaborative UltraHonk prover for the elliptic, memory, non-native field, Poseidon2 external and
Poseidon2 internal relations, restated in Python integers from co-noir/co-ultrahonk/src/co_decider/relations/: the `accumulate` bodies of
elliptic_relation.rs:102-254, memory_relation.rs:166-457, non_native_field_relation.rs:109-215, poseidon2_external_relation.rs:141-228 and
poseidon2_internal_relation.rs:135-227, cut at their mul_many calls, with fold_accumulator! (relations/mod.rs:45-57) at the end of each.
Written in the reference's shape -- whole batch vectors, one vector operation after another -- where the device evaluates one element at
a time, so that the two can be compared. The batch view, the share-vector operations, `fold` and the in-process networks (PlainNet,
Rep3Net, ShamirNet) are tests/honk_co_relations_ref.py's, imported and not edited; the plain side is tests/honk_gates_ref.py's.

Also here, for the tests only: the driver that makes the reference's call sequence of the five relations (the second half of
accumulate_relation_univariates_batch, co_sumcheck_round.rs:140-218) over a set of stage functions, and the share-wise
batch_over_relations_univariates over all 28 accumulators."""
from tests import honk_co_relations_ref as CO
from tests import honk_gates_ref as G
from tests import honk_relations_ref as R

POINTS = CO.POINTS
View, flat, fold, _fold, halves = CO.View, CO.flat, CO.fold, CO._fold, CO.halves
RELATIONS = G.RELATIONS
STAGE_ACC = {"elliptic": [6, 6], "memory": [6] * 6, "nnf": [6], "poseidon2_external": [7] * 4, "poseidon2_internal": [7] * 4}
assert all(c in CO.SHARED for c in G.WITNESS + G.SHIFTED) and not any(c in CO.SHARED for c in G.PRECOMPUTED + G.SELECTORS)


def _parts(v, vec, count):
    """chunks_exact of a flat product vector -> `count` share vectors"""
    x = v.unflat(vec)
    n7 = len(x) // count
    assert n7 * count == len(x) and n7 == POINTS * v.m
    return [x[i * n7:(i + 1) * n7] for i in range(count)]


def _mulpub(a, b, p):
    return [x * y % p for x, y in zip(a, b)]


# ---- elliptic, elliptic_relation.rs:102-254; v.params = the eight gate parameters ---------------------------------------------------------------
def _ell_cols(v):
    return dict(x_1=v.sh("w_r"), y_1=v.sh("w_o"), x_2=v.sh("w_l_shift"), y_2=v.sh("w_4_shift"), y_3=v.sh("w_o_shift"), x_3=v.sh("w_r_shift"))


def ell_operands(v):
    """-> (lhs, rhs), 7 * 7 m shares each, flat"""
    c = _ell_cols(v)
    x_1, y_1, x_2, y_2, y_3, x_3 = (c[k] for k in ("x_1", "y_1", "x_2", "y_2", "y_3", "x_3"))
    x_diff = v.sub(x_2, x_1)
    y1_plus_y3 = v.add(y_1, y_3)
    y_diff = v.sub(v.scale(y_2, v.pub("q_l")), y_1)
    x1_mul_3 = v.add(v.add(x_1, x_1), x_1)
    lhs = y_1 + y_2 + y_1 + x_diff + y1_plus_y3 + y_diff + x1_mul_3
    rhs = y_1 + y_2 + y_2 + x_diff + x_diff + v.sub(x_3, x_1) + x_1
    return flat(lhs), flat(rhs)


def ell_operands2(v, mul1):
    """mul1 = mul_many(lhs, rhs). -> (lhs, rhs), 5 * 7 m shares each, flat"""
    c = _ell_cols(v)
    x_1, y_1, x_2, y_3, x_3 = (c[k] for k in ("x_1", "y_1", "x_2", "y_3", "x_3"))
    chunks1 = _parts(v, mul1, 7)
    curve_b = v.params[3]
    y1_sqr = chunks1[0]
    y1_sqr_mul_4 = v.add(y1_sqr, y1_sqr)
    y1_sqr_mul_4 = v.add(y1_sqr_mul_4, y1_sqr_mul_4)
    lhs = v.add(v.add(x_3, x_2), x_1) + v.add_pub(y1_sqr, -curve_b % v.p) + v.add(v.add(x_3, x_1), x_1) + chunks1[6] + v.add(y_1, y_1)
    rhs = chunks1[3] + v.add(v.add(x_1, x_1), x_1) + y1_sqr_mul_4 + v.sub(x_1, x_3) + v.add(y_1, y_3)
    return flat(lhs), flat(rhs)


def ell_finish(v, mul1, mul2):
    """-> r0 (6) and r1 (6), back to back, flat"""
    p = v.p
    if not v.m:
        return [0] * (12 * v.ncomp)
    chunks1, chunks2 = _parts(v, mul1, 7), _parts(v, mul2, 5)
    q_sign, q_elliptic, q_is_double, sf = v.pub("q_l"), v.pub("q_elliptic"), v.pub("q_m"), v.sf()
    y1_sqr, y2_sqr = chunks1[0], chunks1[1]
    y1y2 = v.scale(chunks1[2], q_sign)
    x_add_identity = v.add(v.add(v.sub(v.sub(chunks2[0], y2_sqr), y1_sqr), y1y2), y1y2)
    q_elliptic_by_scaling = _mulpub(q_elliptic, sf, p)
    q_double = _mulpub(q_elliptic_by_scaling, q_is_double, p)
    q_not_double = [(a - b) % p for a, b in zip(q_elliptic_by_scaling, q_double)]
    tmp_1 = v.scale(x_add_identity, q_not_double)
    tmp_2 = v.scale(v.add(chunks1[4], chunks1[5]), q_not_double)
    x_pow_4_mul_3 = chunks2[1]
    x1_pow_4_mul_9 = v.add(v.add(x_pow_4_mul_3, x_pow_4_mul_3), x_pow_4_mul_3)
    tmp_1 = v.add(tmp_1, v.scale(v.sub(chunks2[2], x1_pow_4_mul_9), q_double))
    tmp_2 = v.add(tmp_2, v.scale(v.sub(chunks2[3], chunks2[4]), q_double))
    return fold(p, tmp_1, 6) + fold(p, tmp_2, 6)


# ---- memory, memory_relation.rs:166-457 ---------------------------------------------------------------------------------------------------------
def _mem_common(v):
    eta, eta_two, eta_three = v.params[:3]
    w = {c: v.sh(c) for c in G.WITNESS + G.SHIFTED}
    memory_record_check = v.scale(w["w_o"], eta_three)
    memory_record_check = v.add(memory_record_check, v.scale(w["w_r"], eta_two))
    memory_record_check = v.add(memory_record_check, v.scale(w["w_l"], eta))
    memory_record_check = v.add_pub(memory_record_check, v.pub("q_c"))
    partial_record_check = list(memory_record_check)
    memory_record_check = v.sub(memory_record_check, w["w_4"])
    neg_index_delta = v.sub(w["w_l"], w["w_l_shift"])
    neg_access_type = v.sub(partial_record_check, w["w_4"])
    neg_next = v.scale(w["w_o_shift"], eta_three)
    neg_next = v.add(neg_next, v.scale(w["w_r_shift"], eta_two))
    neg_next = v.add(neg_next, v.scale(w["w_l_shift"], eta))
    neg_next = v.sub(neg_next, w["w_4_shift"])
    return w, memory_record_check, neg_index_delta, neg_access_type, neg_next


def mem_operands(v):
    """-> (lhs, rhs: 6 * 7 m shares each; rhs2 = neg_next_gate_access_type (+) 1: 7 m shares), flat"""
    w, _, neg_index_delta, neg_access_type, neg_next = _mem_common(v)
    index_delta_is_zero = v.add_pub(neg_index_delta, 1)
    record_delta = v.sub(w["w_4_shift"], w["w_4"])
    value_delta = v.sub(w["w_o_shift"], w["w_o"])
    timestamp_delta = v.sub(w["w_r_shift"], w["w_r"])
    lhs = neg_index_delta + index_delta_is_zero + neg_access_type + index_delta_is_zero + neg_next + index_delta_is_zero
    rhs = neg_index_delta + record_delta + neg_access_type + value_delta + neg_next + timestamp_delta
    return flat(lhs), flat(rhs), flat(v.add_pub(neg_next, 1))


def mem_finish(v, mul, mul2):
    """mul = mul_many(lhs, rhs), mul2 = mul_many(mul[3], rhs2). -> r0 .. r5 (6 each), flat"""
    p = v.p
    if not v.m:
        return [0] * (36 * v.ncomp)
    w, memory_record_check, neg_index_delta, neg_access_type, neg_next = _mem_common(v)
    mul = _parts(v, mul, 6)
    q_1, q_2, q_3, q_4, q_m, q_memory = (v.pub(c) for c in ("q_l", "q_r", "q_o", "q_4", "q_m", "q_memory"))
    sf = v.sf()
    q_memory_by_scaling = _mulpub(sf, q_memory, p)
    q_one_by_two = _mulpub(q_1, q_2, p)
    q_one_by_two_by_memory_by_scaling = _mulpub(q_one_by_two, q_memory_by_scaling, p)
    q_3_by_memory_and_scaling = _mulpub(q_3, q_memory_by_scaling, p)
    rom_consistency_check_identity = v.scale(memory_record_check, q_one_by_two)
    access_check = v.add(mul[2], neg_access_type)
    index_is_monotonically_increasing = v.add(mul[0], neg_index_delta)
    r1 = v.scale(mul[1], q_one_by_two_by_memory_by_scaling)
    r2 = v.scale(index_is_monotonically_increasing, q_one_by_two_by_memory_by_scaling)
    r4 = v.scale(index_is_monotonically_increasing, q_3_by_memory_and_scaling)
    ram_timestamp_check_identity = v.sub(mul[5], w["w_o"])
    next_gate_access_type_is_boolean = v.add(mul[4], neg_next)
    r3 = v.scale(v.unflat(mul2), q_3_by_memory_and_scaling)
    r5 = v.scale(next_gate_access_type_is_boolean, q_3_by_memory_and_scaling)
    ram_consistency_check_identity = v.scale(access_check, q_3_by_memory_and_scaling)
    memory_identity = rom_consistency_check_identity
    memory_identity = v.add(memory_identity, v.scale(ram_timestamp_check_identity, _mulpub(q_4, q_1, p)))
    memory_identity = v.add(memory_identity, v.scale(memory_record_check, _mulpub(q_m, q_1, p)))
    memory_identity = v.scale(memory_identity, q_memory_by_scaling)
    memory_identity = v.add(memory_identity, ram_consistency_check_identity)
    return [a for r in (memory_identity, r1, r2, r3, r4, r5) for a in fold(p, r, 6)]


# ---- non-native field, non_native_field_relation.rs:109-215 -----------------------------------------------------------------------------------
def nnf_operands(v):
    """-> (lhs, rhs), 5 * 7 m shares each, flat"""
    w_1, w_2, w_3, w_4, w_1_shift, w_2_shift = (v.sh(c) for c in ("w_l", "w_r", "w_o", "w_4", "w_l_shift", "w_r_shift"))
    return flat(w_1 + w_2 + w_4 + w_3 + w_1_shift), flat(w_2_shift + w_1_shift + w_1 + w_2 + w_2_shift)


def nnf_finish(v, mul):
    """-> r0 (6), flat"""
    p = v.p
    if not v.m:
        return [0] * (6 * v.ncomp)
    w_1, w_2, w_3, w_4 = (v.sh(c) for c in G.WITNESS)
    w_1_shift, w_2_shift, w_3_shift, w_4_shift = (v.sh(c) for c in G.SHIFTED)
    q_2, q_3, q_4, q_m, q_nnf = (v.pub(c) for c in ("q_r", "q_o", "q_4", "q_m", "q_nnf"))
    limb_size, sublimb_shift = G.LIMB_SIZE % p, G.SUBLIMB_SHIFT % p
    mul = _parts(v, mul, 5)
    limb_subproduct = v.add(mul[0], mul[1])
    gate_2 = v.sub(v.add(mul[2], mul[3]), w_3_shift)
    gate_2 = v.scale(gate_2, limb_size)
    gate_2 = v.sub(gate_2, w_4_shift)
    gate_2 = v.add(gate_2, limb_subproduct)
    gate_2 = v.scale(gate_2, q_4)
    limb_subproduct = v.scale(limb_subproduct, limb_size)
    limb_subproduct = v.add(limb_subproduct, mul[4])
    gate_1 = v.scale(v.sub(v.sub(limb_subproduct, w_3), w_4), q_3)
    gate_3 = v.scale(v.sub(v.sub(v.add(limb_subproduct, w_4), w_3_shift), w_4_shift), q_m)
    identity = v.scale(v.add(v.add(gate_1, gate_2), gate_3), q_2)
    acc_1 = v.scale(w_2_shift, sublimb_shift)
    for t in (w_1_shift, w_3, w_2):
        acc_1 = v.scale(v.add(acc_1, t), sublimb_shift)
    acc_1 = v.scale(v.sub(v.add(acc_1, w_1), w_4), q_4)
    acc_2 = v.scale(w_3_shift, sublimb_shift)
    for t in (w_2_shift, w_1_shift, w_4):
        acc_2 = v.scale(v.add(acc_2, t), sublimb_shift)
    acc_2 = v.scale(v.sub(v.add(acc_2, w_3), w_4_shift), q_m)
    limb_accumulator_identity = v.scale(v.add(acc_1, acc_2), q_3)
    nnf_identity = v.scale(v.scale(v.add(identity, limb_accumulator_identity), q_nnf), v.sf())
    return fold(p, nnf_identity, 6)


# ---- Poseidon2, poseidon2_external_relation.rs:141-228 and poseidon2_internal_relation.rs:135-227 ------------------------------------------------
def pos_ext_operands(v):
    """-> s = [s1 | s2 | s3 | s4], 4 * 7 m shares, flat"""
    return flat([x for w, q in zip(G.WITNESS, ("q_l", "q_r", "q_o", "q_4")) for x in v.add_pub(v.sh(w), v.pub(q))])


def pos_ext_finish(v, u):
    """u = s^5 by three mul_many. -> r0 .. r3, SEVEN each, flat"""
    p = v.p
    if not v.m:
        return [0] * (28 * v.ncomp)
    u = _parts(v, u, 4)
    t0 = v.add(u[0], u[1])
    t1 = v.add(u[2], u[3])
    t2 = v.add(v.add(u[1], u[1]), t1)
    t3 = v.add(v.add(u[3], u[3]), t0)
    v4 = v.add(t1, t1)
    v4 = v.add(v.add(v4, v4), t3)
    v2 = v.add(t0, t0)
    v2 = v.add(v.add(v2, v2), t2)
    v1 = v.add(t3, v2)
    v3 = v.add(t2, v4)
    q_pos_by_scaling = _mulpub(v.pub("q_poseidon2_external"), v.sf(), p)
    return [a for x, ws in zip((v1, v2, v3, v4), G.SHIFTED) for a in fold(p, v.scale(v.sub(x, v.sh(ws)), q_pos_by_scaling), 7)]


def pos_int_operands(v):
    """-> s1, 7 m shares, flat"""
    return flat(v.add_pub(v.sh("w_l"), v.pub("q_l")))


def pos_int_finish(v, u1):
    """u1 = s1^5. -> r0 .. r3, SEVEN each, flat"""
    p = v.p
    if not v.m:
        return [0] * (28 * v.ncomp)
    u = [v.unflat(u1), v.sh("w_r"), v.sh("w_o"), v.sh("w_4")]
    total = v.add(v.add(v.add(u[0], u[1]), u[2]), u[3])
    q_pos_by_scaling = _mulpub(v.pub("q_poseidon2_internal"), v.sf(), p)
    out = []
    for i in range(4):
        x = v.sub(v.add(v.scale(u[i], v.params[4 + i]), total), v.sh(G.SHIFTED[i]))
        out += fold(p, v.scale(x, q_pos_by_scaling), 7)
    return out


# ---- the parties' views, the stage functions and the round -------------------------------------------------------------------------------------
def select_lists(pub_polys, edge_begin, edge_end):
    """can_skip of the five relations: each by its own selector"""
    return {rel: CO.select_edges(pub_polys, G.SELECTOR_OF[rel], edge_begin, edge_end) for rel in RELATIONS}


def make_views(p, party_polys, protocol, gate_params, edge_begin, edge_end, scaling=None, stride=1, lists=None):
    """views[rel][party] over the 19 (or more) columns; every relation takes the edge list of its selector"""
    lists = lists or select_lists(party_polys[0], edge_begin, edge_end)
    return {rel: [View(p, polys, protocol, i, gate_params, edge_begin, edge_end, lists[rel], scaling, stride) for i, polys in enumerate(party_polys)]
            for rel in RELATIONS}


class RefStages:
    """the stage functions of this module over the parties' views: views[rel][party]"""
    STAGES = {"ell_operands": (ell_operands, "elliptic"), "ell_operands2": (ell_operands2, "elliptic"), "ell_finish": (ell_finish, "elliptic"),
              "mem_operands": (mem_operands, "memory"), "mem_finish": (mem_finish, "memory"), "nnf_operands": (nnf_operands, "nnf"),
              "nnf_finish": (nnf_finish, "nnf"), "pos_ext_operands": (pos_ext_operands, "poseidon2_external"),
              "pos_ext_finish": (pos_ext_finish, "poseidon2_external"), "pos_int_operands": (pos_int_operands, "poseidon2_internal"),
              "pos_int_finish": (pos_int_finish, "poseidon2_internal")}

    def __init__(self, views):
        self.views = views

    def m(self, rel):
        return self.views[rel][0].m

    def __getattr__(self, name):
        if name not in self.STAGES:
            raise AttributeError(name)
        fn, rel = self.STAGES[name]
        return lambda i, *args: fn(self.views[rel][i], *args)


Both = CO.Both


def _sbox(net, s):
    """x^5 as the reference does it: three mul_many"""
    u = net.mul_many(s, s)
    u = net.mul_many(u, u)
    return net.mul_many(u, s)


def run_round_gates(net, st):
    """accumulate_relation_univariates_batch (co_sumcheck_round.rs:140-218) for the elliptic, memory, nnf, Poseidon2 external and internal
    relations in that order, every party in turn; a relation without kept edges makes no network call and leaves zeros. -> per party the
    seventeen accumulators (flat share lists) in subrelation order"""
    P = range(net.n)
    nc = net.protocol + 1
    empty = [[] for _ in P]
    acc = [[] for _ in P]

    def split(i, out, lens):
        at = 0
        for ln in lens:
            acc[i].append(out[at:at + ln * nc])
            at += ln * nc
        assert at == len(out)

    # elliptic
    if st.m("elliptic"):
        ops = [st.ell_operands(i) for i in P]
        mul1 = net.mul_many([o[0] for o in ops], [o[1] for o in ops])
        ops = [st.ell_operands2(i, mul1[i]) for i in P]
        mul2 = net.mul_many([o[0] for o in ops], [o[1] for o in ops])
    else:
        mul1 = mul2 = empty
    for i in P:
        split(i, st.ell_finish(i, mul1[i], mul2[i]), STAGE_ACC["elliptic"])
    # memory
    if st.m("memory"):
        ops = [st.mem_operands(i) for i in P]
        mul = net.mul_many([o[0] for o in ops], [o[1] for o in ops])
        n7 = len(mul[0]) // 6
        mul2 = net.mul_many([x[3 * n7:4 * n7] for x in mul], [o[2] for o in ops])
    else:
        mul = mul2 = empty
    for i in P:
        split(i, st.mem_finish(i, mul[i], mul2[i]), STAGE_ACC["memory"])
    # nnf
    if st.m("nnf"):
        ops = [st.nnf_operands(i) for i in P]
        mul = net.mul_many([o[0] for o in ops], [o[1] for o in ops])
    else:
        mul = empty
    for i in P:
        split(i, st.nnf_finish(i, mul[i]), STAGE_ACC["nnf"])
    # Poseidon2
    u = _sbox(net, [st.pos_ext_operands(i) for i in P]) if st.m("poseidon2_external") else empty
    for i in P:
        split(i, st.pos_ext_finish(i, u[i]), STAGE_ACC["poseidon2_external"])
    u = _sbox(net, [st.pos_int_operands(i) for i in P]) if st.m("poseidon2_internal") else empty
    for i in P:
        split(i, st.pos_int_finish(i, u[i]), STAGE_ACC["poseidon2_internal"])
    return acc


def open_round_gates(net, acc):
    """-> the seventeen opened accumulators"""
    return [net.open([acc[i][s] for i in range(net.n)]) for s in range(len(G.ACC_LEN))]


def batch_over_relations_shares_all(p, acc, ncomp, alphas, current_element, partial_evaluation_result):
    """batch_over_relations_univariates on one party's shares of all 28 accumulators (co_sumcheck_round.rs:121-138): linear in the
    shares, so component by component. -> 8 shares, flat"""
    out = [0] * (R.BATCHED_RELATION_PARTIAL_LENGTH * ncomp)
    for cc in range(ncomp):
        out[cc::ncomp] = G.batch_over_relations_univariates_all(p, [a[cc::ncomp] for a in acc], alphas, current_element, partial_evaluation_result)
    return out
