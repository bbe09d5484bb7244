"""Big-integer restatement of the Poseidon2 gadget of the reference (mpc-core/src/gadgets/poseidon2/poseidon2_permutation.rs, rep3.rs,
shamir.rs and gadgets/merkle_tree/{plain,rep3,shamir}.rs), d = 5, t = 2, 3, 4: the plain permutation, both Merkle trees, and the packed
permutation with precomputation of three Rep3 or Shamir parties simulated in one process. The collaborative permutation is written in the
step form of csh_poseidon2_co_round_dev (post-part of round s - 1, pre-part of round s), so that the same driver runs the restatement
and the device entries. Parameter sets come from a seeded generator of the tests' own: nothing here is a real Poseidon2 instance.
tests/test_poseidon2_cpu.py is what makes this file a reference."""
import random
from collections import namedtuple

Params = namedtuple("Params", "p t rf_b rf_e rp rc_ext rc_int diag")
SHAPES = {"bn254": (4, 4, 56), "short": (2, 2, 3)}   # the reference's BN254 round numbers; a short set on which index errors show
SPONGE, COMPRESSION = 0, 1


def make_params(p, t, shape, seed=1):
    """a seeded parameter set; t = 2, 3 carry the diagonals the fixed internal matrices stand for, t = 4 four distinct values"""
    rf_b, rf_e, rp = SHAPES[shape]
    r = random.Random("poseidon2/%d/%s/%d/%d" % (t, shape, seed, p))
    rc_ext = [[r.randrange(p) for _ in range(t)] for _ in range(rf_b + rf_e)]
    rc_int = [r.randrange(p) for _ in range(rp)]
    diag = {2: [1, 2], 3: [1, 1, 2]}.get(t) or [r.randrange(3, p) for _ in range(4)]
    assert len(set(diag)) == len(diag) or t < 4
    return Params(p, t, rf_b, rf_e, rp, rc_ext, rc_int, diag)


def rounds(P):
    return P.rf_b + P.rp + P.rf_e


def num_sbox(P):
    return (P.rf_b + P.rf_e) * P.t + P.rp


def is_external(P, r):
    return r < P.rf_b or r >= P.rf_b + P.rp


def rc_of(P, r):
    """round r's constants per s-box position: the end rounds read on from index rounds_f_beginning (poseidon2_permutation.rs:209-213)"""
    if r < P.rf_b:
        return P.rc_ext[r]
    if r < P.rf_b + P.rp:
        return [P.rc_int[r - P.rf_b]]
    return P.rc_ext[r - P.rp]


# ---- linear layers on anything with +: ints mod p here, share components below --------------------------------------------------------------
def matmul_m4(x, p):
    """poseidon2_permutation.rs:67-80"""
    t0 = x[0] + x[1]
    t1 = x[2] + x[3]
    t2 = 2 * x[1] + t1
    t3 = 2 * x[3] + t0
    t4 = 4 * t1 + t3
    t5 = 4 * t0 + t2
    t6 = t3 + t5
    t7 = t2 + t4
    return [t6 % p, t5 % p, t7 % p, t4 % p]


def matmul_external(x, p):
    """:83-123"""
    if len(x) == 4:
        return matmul_m4(x, p)
    s = sum(x)
    return [(v + s) % p for v in x]


def matmul_internal(P, x):
    """:126-162"""
    p, s = P.p, sum(x)
    if P.t == 2:
        return [(x[0] + s) % p, (2 * x[1] + s) % p]
    if P.t == 3:
        return [(x[0] + s) % p, (x[1] + s) % p, (2 * x[2] + s) % p]
    return [(v * d + s) % p for v, d in zip(x, P.diag)]


def permutation(P, state):
    """permutation_in_place (:194-214)"""
    p = P.p
    x = matmul_external(list(state), p)
    for r in range(P.rf_b):
        x = matmul_external([pow(v + c, 5, p) for v, c in zip(x, P.rc_ext[r])], p)
    for r in range(P.rp):
        x[0] = pow(x[0] + P.rc_int[r], 5, p)
        x = matmul_internal(P, x)
    for r in range(P.rf_b, P.rf_b + P.rf_e):
        x = matmul_external([pow(v + c, 5, p) for v, c in zip(x, P.rc_ext[r])], p)
    return x


def permute_batch(P, flat):
    out = []
    for i in range(0, len(flat), P.t):
        out += permutation(P, flat[i:i + P.t])
    return out


# ---- Merkle trees, plain (merkle_tree/plain.rs) ------------------------------------------------------------------------------------------
def _power_of(n, arity):
    while n > 1 and n % arity == 0:
        n //= arity
    return n == 1


def merkle_tree(P, leaves, arity, mode):
    """merkle_tree_sponge (:15-50) and merkle_tree_compression (:113-155), the flat buffer and its index arithmetic kept"""
    T, p = P.t, P.p
    assert (T > arity) if mode == SPONGE else (T >= arity)
    ln = len(leaves)
    assert _power_of(ln, arity)
    if mode == COMPRESSION and T == arity:
        buf = list(leaves)
    else:
        buf = []
        for i in range(0, ln, arity):
            buf += list(leaves[i:i + arity]) + [0] * (T - arity)
    while ln > 1:
        ln //= arity
        for k in range(ln):
            ff = buf[T * k]
            buf[T * k:T * k + T] = permutation(P, buf[T * k:T * k + T])
            if mode == COMPRESSION:
                buf[T * k] = (buf[T * k] + ff) % p
        for i in range(ln // arity):
            for j in range(arity):
                buf[T * i + j] = buf[T * arity * i + j * T]
            for j in range(arity, T):
                buf[T * i + j] = 0
    return buf[0]


def trivial_merkle_tree(P, leaves, arity, mode):
    """every node hashed separately (trivial_merkle_tree_sponge / _compression, :308-369)"""
    layer = list(leaves)
    while len(layer) > 1:
        nxt = []
        for i in range(0, len(layer), arity):
            st = layer[i:i + arity] + [0] * (P.t - arity)
            h = permutation(P, st)[0]
            nxt.append((h + st[0]) % P.p if mode == COMPRESSION else h)
        layer = nxt
    return layer[0]


def num_hashes(n_leaves, arity):
    return (n_leaves - 1) // (arity - 1)


# ---- parties ---------------------------------------------------------------------------------------------------------------------------------
# A share is a tuple of ncomp = protocol + 1 ints. Rep3: (a, b), x = a_0 + a_1 + a_2, b_i = a_(i-1) (rep3.rs:281-292). Shamir: degree 1
# over three parties at the points 1, 2, 3 (shamir.rs:359-376). Plain: the value itself.
def pub_comp(protocol, party):
    """the component that takes a public value: x (+) v"""
    return 0 if protocol == 0 else {0: 0, 1: 1}.get(party, -1)


class Rep3Net:
    n, protocol, kind = 3, 1, "rep3"

    def __init__(self, p):
        self.p = p

    def share(self, vals, rnd):
        out = [[], [], []]
        for v in vals:
            a, b = rnd.randrange(self.p), rnd.randrange(self.p)
            c = (v - a - b) % self.p
            for k, s in enumerate(((a, c), (b, a), (c, b))):
                out[k].append(s)
        return out

    def open(self, per_party):
        """open_vec (rep3/arithmetic.rs:249-271): a + b + the previous party's b; every party gets the same values"""
        p0, p1, p2 = per_party
        vals = [(x[0] + x[1] + z[1]) % self.p for x, z in zip(p0, p2)]
        assert vals == [(x[0] + y[0] + z[0]) % self.p for x, y, z in zip(p0, p1, p2)]
        return vals


class ShamirNet:
    n, protocol, kind = 3, 0, "shamir"

    def __init__(self, p):
        self.p = p
        self.lagrange = []
        for i in (1, 2, 3):
            num = den = 1
            for j in (1, 2, 3):
                if j != i:
                    num, den = num * j % p, den * (j - i) % p
            self.lagrange.append(num * pow(den, -1, p) % p)

    def share(self, vals, rnd):
        out = [[], [], []]
        for v in vals:
            c1 = rnd.randrange(self.p)
            for k in range(3):
                out[k].append(((v + c1 * (k + 1)) % self.p,))
        return out

    def open(self, per_party):
        return [sum(s[0] * l for s, l in zip(col, self.lagrange)) % self.p for col in zip(*per_party)]


class PlainNet:
    n, protocol, kind = 1, 0, "plain"

    def __init__(self, p):
        self.p = p

    def share(self, vals, rnd):
        return [[(v % self.p,) for v in vals]]

    def open(self, per_party):
        return [s[0] for s in per_party[0]]


NETS = {"rep3": Rep3Net, "shamir": ShamirNet, "plain": PlainNet}


def precompute(P, net, n_perm, rnd):
    """precompute_rep3 / precompute_shamir (rep3.rs:12-51, shamir.rs:35-73): per party the five share vectors r, r^2, r^3, r^4, r^5 of
    num_sbox * n_perm entries. The products of the reference are multiplications with a reshare, i.e. fresh sharings of the powers."""
    r = [rnd.randrange(P.p) for _ in range(num_sbox(P) * n_perm)]
    vecs = [net.share([pow(v, k, P.p) for v in r], rnd) for k in range(1, 6)]
    return [[vecs[k][party] for k in range(5)] for party in range(net.n)]


def _addpub(p, share, v, pc):
    return tuple((c + v) % p if k == pc else c for k, c in enumerate(share))


def sbox_post(p, y, r, pc):
    """sbox_rep3_precomp_post (rep3.rs:358-388), sbox_shamir_precomp_post (shamir.rs:137-153): r = the entry's five shares"""
    y2 = y * y % p
    y3, y4 = y2 * y % p, y2 * y2 % p
    res = tuple((c5 + 5 * y * c4 + 10 * y2 * c3 + 10 * y3 * c2 + 5 * y4 * c1) % p for c1, c2, c3, c4, c5 in zip(*r))
    return _addpub(p, res, y4 * y % p, pc)


def co_step(P, protocol, party, step, state, n_perm, y, pre, off):
    """One party's local stretch: the post-part of round step - 1 and the pre-part of round step, as csh_poseidon2_co_round_dev
    defines them. state: n_perm * t shares; y: the opened values of round step - 1; pre: the party's five vectors; off: the offset of
    round `step` (at step R: the offset after the last round). -> (state after the linear layer, the shares to open, feed-forward)."""
    p, T, R, pc = P.p, P.t, rounds(P), pub_comp(protocol, party)
    nc = protocol + 1
    lin = lambda f, st: [tuple(col) for col in zip(*[f([s[c] for s in st]) for c in range(nc)])]
    st, ff = list(state), None
    if step == 0:
        ff = [st[i * T] for i in range(n_perm)]
        for i in range(n_perm):
            st[i * T:(i + 1) * T] = lin(lambda x: matmul_external(x, p), st[i * T:(i + 1) * T])
    else:
        r = step - 1
        if is_external(P, r):
            base = off - n_perm * T
            for i in range(n_perm):
                blk = [sbox_post(p, y[i * T + j], [pre[k][base + i * T + j] for k in range(5)], pc) for j in range(T)]
                st[i * T:(i + 1) * T] = lin(lambda x: matmul_external(x, p), blk)
        else:
            base = off - n_perm
            for i in range(n_perm):
                blk = [sbox_post(p, y[i], [pre[k][base + i] for k in range(5)], pc)] + st[i * T + 1:(i + 1) * T]
                st[i * T:(i + 1) * T] = lin(lambda x: matmul_internal(P, x), blk)
    opened = []
    if step < R:
        rc = rc_of(P, step)
        pos = range(T) if is_external(P, step) else range(1)
        for i in range(n_perm):
            for j in pos:
                idx = off + (i * T + j if is_external(P, step) else i)
                v = _addpub(p, st[i * T + j], rc[j], pc)
                opened.append(tuple((a - b) % p for a, b in zip(v, pre[0][idx])))
    return st, opened, ff


class RefStepper:
    """the restatement's co_step behind the interface the device tests substitute"""

    def __init__(self, P, net):
        self.P, self.net = P, net

    def step(self, party, step, state, n_perm, y, pre, off):
        return co_step(self.P, self.net.protocol, party, step, state, n_perm, y, pre, off)

    def layer_next(self, party, state, ff, arity, mode, ln):
        return layer_next(self.P, state, ff, arity, mode, ln)


def round_entries(P, r, n_perm):
    return n_perm * P.t if is_external(P, r) else n_perm


def co_permutation(P, net, stepper, states, pre, off):
    """*_permutation_in_place_with_precomputation_packed (rep3.rs:612-648, shamir.rs:326-365) through R + 1 steps with an opening between
    two of them. states / pre: per party. -> (states per party, the offset after it, feed-forwards per party)"""
    n_perm = len(states[0]) // P.t
    y, ffs = None, None
    for s in range(rounds(P) + 1):
        res = [stepper.step(k, s, states[k], n_perm, y, pre[k], off) for k in range(net.n)]
        states = [r[0] for r in res]
        if s == 0:
            ffs = [r[2] for r in res]
        if s < rounds(P):
            y = net.open([r[1] for r in res])
            off += round_entries(P, s, n_perm)
    return states, off, ffs


def layer_next(P, state, ff, arity, mode, ln):
    """the gather after a layer of ln states (merkle_tree/rep3.rs:44-52, :99-111): csh_poseidon2_layer_next_dev"""
    p, T = P.p, P.t
    zero = tuple(0 for _ in state[0])
    el = lambda k: tuple((a + b) % p for a, b in zip(state[k * T], ff[k])) if mode == COMPRESSION else state[k * T]
    if ln == 1:
        return [el(0)]
    out = []
    for i in range(ln // arity):
        out += [el(arity * i + j) for j in range(arity)] + [zero] * (T - arity)
    return out


def co_merkle_tree(P, net, stepper, leaves, arity, mode, pre):
    """merkle_tree_sponge_rep3 / _compression_rep3 (merkle_tree/rep3.rs) and their Shamir forms: leaves and pre per party.
    -> (the root's share per party, the final precomputation offset)"""
    T = P.t
    ln = len(leaves[0])
    assert _power_of(ln, arity) and ln > 1
    zero = tuple(0 for _ in leaves[0][0])
    states = []
    for lv in leaves:
        buf = []
        for i in range(0, ln, arity):
            buf += list(lv[i:i + arity]) + [zero] * (T - arity)
        states.append(buf)
    off = 0
    while ln > 1:
        ln //= arity
        states, off, ffs = co_permutation(P, net, stepper, [s[:T * ln] for s in states], pre, off)
        states = [stepper.layer_next(k, states[k], ffs[k], arity, mode, ln) for k in range(net.n)]
    return [s[0] for s in states], off
