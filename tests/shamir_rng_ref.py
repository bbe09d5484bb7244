"""Big-integer restatement of the Shamir preprocessing of mpc-core (test infrastructure only; it calls nothing of the library).

  * `Stream`: F::rand and 32-byte seed draws over ChaCha12Rng::from_seed(seed), positions counted in 32-byte candidates. The sampling
    rule is that of oracle.arkfmt.expand_seeded (ark-ff 0.6.0 restated, PARITY UNPINNED: no reference vector); `field_rand_ref` is
    held against expand_seeded itself in tests/test_shamir_rng_cpu.py. The keystream comes from a vectorised copy of oracle.chacha.block,
    held against it in the same file.
  * `ShamirRngRef`: random_double_share, buffer_triples, get_pair and fork_with_pairs of mpc-core/src/protocols/shamir/rngs.rs,
    written the way the reference writes them -- per-item vectors rcv[b][0 .. n), coefficient polynomials, one loop after another -- in
    the two-stage form of the C entries (`local` ends with send_share_of_randomness, `finish` begins with receive_share_of_randomness).
  * `get_shared_rngs`, `run_double_share`: n parties in one process over an in-process network (FIFO queues per ordered pair). The
    driver takes any objects with local / finish, so the same code drives the restatement and the device.

Values are canonical integers mod p; a draw's raw limbs are the Montgomery representation, so its value is limbs * R^-1 and
helpers.pack of the value gives the raw limbs back."""
from __future__ import annotations

import numpy as np

from oracle import chacha

_U32 = np.uint32


def _rotl(v, c):
    return (v << _U32(c)) | (v >> _U32(32 - c))


def chacha12_blocks(key: bytes, first: int, count: int) -> np.ndarray:
    """blocks first .. first + count of the ChaCha12 keystream as a (count, 64) uint8 array (oracle.chacha.block, vectorised)"""
    k = np.frombuffer(key, dtype="<u4")
    ctr = np.arange(first, first + count, dtype=np.uint64)
    st = [np.full(count, c, dtype=_U32) for c in (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)]
    st += [np.full(count, int(w), dtype=_U32) for w in k]
    st += [(ctr & np.uint64(0xFFFFFFFF)).astype(_U32), (ctr >> np.uint64(32)).astype(_U32), np.zeros(count, dtype=_U32), np.zeros(count, dtype=_U32)]
    x = [a.copy() for a in st]

    def qr(a, b, c, d):
        x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 16)
        x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 12)
        x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 8)
        x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 7)

    with np.errstate(over="ignore"):
        for _ in range(6):
            qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
            qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
        words = np.stack([a + b for a, b in zip(x, st)], axis=1).astype("<u4")
    return words.view(np.uint8).reshape(count, 64)


def candidates(key: bytes, begin: int, count: int):
    """the unmasked 256-bit little-endian integers of candidates begin .. begin + count"""
    b0 = begin >> 1
    raw = chacha12_blocks(key, b0, ((begin + count + 1) >> 1) - b0).reshape(-1, 32)
    off = begin - 2 * b0
    return [int.from_bytes(raw[off + i].tobytes(), "little") for i in range(count)]


def accepted(F, v: int):
    """masked candidate if it is accepted, else None"""
    v &= (1 << F.p.bit_length()) - 1
    return v if v < F.p else None


def field_rand_ref(F, seed: bytes, cand_begin: int, n: int):
    """-> (raw limbs values of the first n accepted candidates at or after cand_begin, index one past the last candidate consumed)"""
    out, pos = [], cand_begin
    while len(out) < n:
        step = max(64, 2 * (n - len(out)))
        for v in candidates(seed, pos, step):
            pos += 1
            a = accepted(F, v)
            if a is not None:
                out.append(a)
                if len(out) == n:
                    break
    return out, pos


class Stream:
    """ChaCha12Rng::from_seed(seed) as the reference uses it: F::rand and gen::<[u8; 32]>(); pos counts candidates"""

    def __init__(self, F, seed: bytes, pos: int = 0):
        self.F, self.seed, self.pos = F, bytes(seed), pos
        self._lo, self._buf = 0, []

    def _cand(self, k):
        if not self._lo <= k < self._lo + len(self._buf):
            self._lo, self._buf = k, candidates(self.seed, k, 512)
        return self._buf[k - self._lo]

    def rand(self) -> int:
        while True:
            a = accepted(self.F, self._cand(self.pos))
            self.pos += 1
            if a is not None:
                return a * self.F.Rinv % self.F.p

    def gen_seed(self) -> bytes:
        v = self._cand(self.pos)
        self.pos += 1
        return v.to_bytes(32, "little")


# ---- shamir.rs ---------------------------------------------------------------------------------------------------------------------------
def evaluate_poly(F, poly, x):
    ev = poly[-1]
    for c in reversed(poly[:-1]):
        ev = (ev * x + c) % F.p
    return ev


def lagrange_from_coeff(F, coeffs):
    res = []
    for i in coeffs:
        num = den = 1
        for j in coeffs:
            if i != j:
                num = num * j % F.p
                den = den * (j - i) % F.p
        res.append(num * pow(den, -1, F.p) % F.p)
    return res


def _poly_times_root_inplace(F, poly, root):
    poly.insert(0, 0)
    for i in range(1, len(poly)):
        poly[i - 1] = (poly[i - 1] - poly[i] * root) % F.p


def precompute_interpolation_polys(F, coeffs):
    res = []
    for i in coeffs:
        num, d = [1], 1
        for j in coeffs:
            if i != j:
                _poly_times_root_inplace(F, num, j)
                d = d * (i - j) % F.p
        c = pow(d, -1, F.p)
        res.append([r * c % F.p for r in num])
    return res


def interpolate_poly_from_precomputed(F, shares, precomputed):
    res = [0] * len(shares)
    for i, p in zip(precomputed, shares):
        for k, n in enumerate(i):
            res[k] = (res[k] + n * p) % F.p
    return res


def send_ids(pid, n, t):
    """receivers of send_share_of_randomness in wire order: the t block (seeded = t + 1), then the 2t block (seeded = 2t)"""
    return [(pid + i + t + 1) % n for i in range(1, n - t - 1)] + [(pid + i + 2 * t) % n for i in range(1, n - 2 * t)]


def recv_ids(pid, n, t):
    """senders of receive_share_of_randomness in its order"""
    return [(pid + n - (t + 1) - i) % n for i in range(1, n - t - 1)] + [(pid + n - 2 * t - i) % n for i in range(1, n - 2 * t)]


# ---- shamir/rngs.rs ----------------------------------------------------------------------------------------------------------------------
class ShamirRngRef:
    def __init__(self, F, pid, num_parties, threshold, shared_rngs, rng=None):
        if 2 * threshold + 1 > num_parties:
            raise ValueError("Threshold too large for number of parties")
        self.F, self.id, self.num_parties, self.threshold = F, pid, num_parties, threshold
        self.shared_rngs, self.rng = shared_rngs, rng
        self.matrix = [[pow(col, row, F.p) for col in range(1, num_parties + 1)] for row in range(threshold + 1)]  # create_vandermonde_matrix
        self.pre_t = precompute_interpolation_polys(F, [(pid + i) % num_parties + 1 for i in range(1, threshold + 2)])
        self.pre_2t = precompute_interpolation_polys(F, [0] + [(pid + i) % num_parties + 1 for i in range(1, 2 * threshold + 1)])
        self.r_t, self.r_2t = [], []
        self._rcv = None

    def positions(self):
        return [s.pos for s in self.shared_rngs]

    def get_rng_mut(self, other):
        return self.shared_rngs[other] if other < self.id else self.shared_rngs[other - 1] if other > self.id else self.rng

    def _receive_seeded(self, degree, output, nxt):
        for i in range(1, degree + 1):
            send_id = (self.id + self.num_parties - i) % self.num_parties
            if (send_id < self.id) if nxt else (send_id > self.id):
                continue
            rng = self.get_rng_mut(send_id)
            for r in output:
                r[send_id] = rng.rand()

    def _send_share_of_randomness(self, seeded, polys):
        out = []
        for i in range(1, self.num_parties - seeded):
            rcv_id = (self.id + i + seeded) % self.num_parties
            out.append([evaluate_poly(self.F, p, rcv_id + 1) for p in polys])
        return out

    def local(self, amount):
        """random_double_share up to send_share_of_randomness -> the wire vectors, in order"""
        F, n, t = self.F, self.num_parties, self.threshold
        rcv_t = [[0] * n for _ in range(amount)]
        rcv_2t = [[0] * n for _ in range(amount)]
        self._receive_seeded(t + 1, rcv_t, True)
        shares = [[0] * (t + 1) for _ in range(amount)]
        for i in range(1, t + 2):
            rng = self.get_rng_mut((self.id + i) % n)
            for s in shares:
                s[i - 1] = rng.rand()
        self._receive_seeded(t + 1, rcv_t, False)
        polys_t = [interpolate_poly_from_precomputed(F, s, self.pre_t) for s in shares]
        rands = []
        for r, p in zip(rcv_t, polys_t):
            r[self.id] = evaluate_poly(F, p, self.id + 1)
            rands.append(p[0])
        self._receive_seeded(2 * t, rcv_2t, True)
        shares = [[r] for r in rands]  # get_interpolation_polys_from_precomputed::<false>
        for i in range(1, 2 * t + 1):
            rng = self.get_rng_mut((self.id + i) % n)
            for s in shares:
                s.append(rng.rand())
        polys_2t = [interpolate_poly_from_precomputed(F, s, self.pre_2t) for s in shares]
        self._receive_seeded(2 * t, rcv_2t, False)
        for r, p in zip(rcv_2t, polys_2t):  # set_my_share
            r[self.id] = evaluate_poly(F, p, self.id + 1)
        self._rcv = (rcv_t, rcv_2t)
        return self._send_share_of_randomness(t + 1, polys_t) + self._send_share_of_randomness(2 * t, polys_2t)

    def finish(self, amount, received):
        """receive_share_of_randomness, then buffer_triples' matmul; `received`: the vectors in the order of recv_ids"""
        n, t = self.num_parties, self.threshold
        rcv_t, rcv_2t = self._rcv
        assert len(rcv_t) == amount
        it = iter(received)
        for seeded, output in ((t + 1, rcv_t), (2 * t, rcv_2t)):
            for i in range(1, n - seeded):
                send_id = (self.id + n - seeded - i) % n
                for r, s in zip(output, next(it)):
                    r[send_id] = s
        for buf, rcv in ((self.r_t, rcv_t), (self.r_2t, rcv_2t)):
            for src in rcv:
                buf.extend(sum(v * cell for v, cell in zip(src, row)) % self.F.p for row in self.matrix)
        self._rcv = None

    def get_pair(self):
        return self.r_t.pop(), self.r_2t.pop()

    def fork_with_pairs(self, amount):
        rng = Stream(self.F, self.rng.gen_seed()) if self.rng is not None else None
        shared = [Stream(self.F, s.gen_seed()) for s in self.shared_rngs]
        if amount > len(self.r_t):
            raise ValueError("not enough corr rand pairs")
        child = ShamirRngRef(self.F, self.id, self.num_parties, self.threshold, shared, rng)
        child.r_t, self.r_t = self.r_t[:amount], self.r_t[amount:]
        child.r_2t, self.r_2t = self.r_2t[:amount], self.r_2t[amount:]
        return child


def get_shared_rngs(F, num_parties, own_seeds):
    """ShamirRng::get_shared_rngs for every party over an in-process network -> (own rngs, per party the num_parties - 1 shared seeds)"""
    rngs = [Stream(F, s) for s in own_seeds]
    seeds = [[None] * num_parties for _ in range(num_parties)]
    wire = {}
    def sends(pid):
        send = (num_parties - 1) // 2
        return send + 1 if (num_parties - 1) & 1 == 1 and pid < num_parties // 2 else send

    for pid in range(num_parties):
        for id_off in range(1, sends(pid) + 1):
            rcv_id = (pid + id_off) % num_parties
            seeds[pid][rcv_id] = wire[(pid, rcv_id)] = rngs[pid].gen_seed()
    for pid in range(num_parties):
        for id_off in range(1, num_parties - 1 - sends(pid) + 1):
            send_id = (pid + num_parties - id_off) % num_parties
            seeds[pid][send_id] = wire[(send_id, pid)]
    shared = []
    for pid in range(num_parties):
        assert seeds[pid][pid] is None and all(s is not None for k, s in enumerate(seeds[pid]) if k != pid)
        shared.append(seeds[pid][:pid] + seeds[pid][pid + 1:])
    return rngs, shared


def run_double_share(parties, amount, n, t):
    """One buffer_triples(amount) of every party over FIFO queues -> per party (wire vectors sent, vectors received)"""
    queues, sent, got = {}, [], []
    for pid, p in enumerate(parties):
        vecs = p.local(amount)
        sent.append(vecs)
        for dst, v in zip(send_ids(pid, n, t), vecs):
            queues.setdefault((pid, dst), []).append(v)
    for pid, p in enumerate(parties):
        rec = [queues[(src, pid)].pop(0) for src in recv_ids(pid, n, t)]
        got.append(rec)
        p.finish(amount, rec)
    assert all(not q for q in queues.values())
    return sent, got


def make_parties(F, n, t, master: bytes):
    """n restatement parties with shared streams from get_shared_rngs; own seeds = candidates of the stream `master`"""
    m = Stream(F, master)
    own = [m.gen_seed() for _ in range(n)]
    rngs, shared = get_shared_rngs(F, n, own)
    return [ShamirRngRef(F, pid, n, t, [Stream(F, s) for s in shared[pid]], rngs[pid]) for pid in range(n)], shared


def open_pairs(F, parties, n, t, ring_of):
    """(values from the degree-t shares, values from the degree-2t shares) with open_lagrange_t / open_lagrange_2t of party ring_of"""
    out = []
    for deg, bufs in ((t, [p.r_t for p in parties]), (2 * t, [p.r_2t for p in parties])):
        ids = [(ring_of + n - i) % n for i in range(deg + 1)]
        lag = lagrange_from_coeff(F, [i + 1 for i in ids])
        out.append([sum(l * bufs[i][k] for l, i in zip(lag, ids)) % F.p for k in range(len(bufs[0]))])
    return out
