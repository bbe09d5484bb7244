"""Plain reference of the MSM sort stage (k_msm_digits + msm_sort.hip, or msm_sort_wide.hip with its own wide_codes), written from the
definition in numpy and vectorised over the scalars: one numpy step per window on the four 64-bit limbs.

  digits     scalar = sum_w d_w 2^(offset_w) with |d_w| <= half_w = 2^(width_w - 1): the chunk of width_w bits at offset_w plus the carry
             of the window below, negative (chunk + carry - 2^width_w, carry out) when chunk + carry > half_w. The low `wide` windows
             are c bits wide, the others c - 1 (balanced plans; wide == W: uniform). Every call checks its own result: the sum above
             is rebuilt in 32-bit columns and compared with the scalar, and |d_w| <= half_w.
  filing     sort window w' of W' holds the digits of the windows w = k W' + w' (k = table row, one row for plain plans). A non-zero
             digit of scalar i is the entry id | sign << 31 in bucket |d_w|, id = k stride + offset + i (tables) or i (plain).
  outputs    per sort window: start[0] = 0, start[b] = first slot of bucket b (1 .. NB), start[NB + 1] = entries of the window;
             nlanes = ceil(entries / lane length of the window); the entries in (bucket, entry) order.

It calls nothing of the library: the host recoder (csh_selftest_digits) is compared with it in tests/test_msm_sort_ref_cpu.py, the two
device recoders and the sorts in tests/test_gpu_msm_sort.py. Scalars are canonical integers below the field's modulus."""
import random
from collections import namedtuple

import numpy as np

U64 = np.uint64

# the words csh_selftest_msm_sort_dev reports (selftest_dev.hip SI_*), in order
INFO_FIELDS = ("c", "W", "wide", "NB", "L", "Ln", "dig_g", "dig_wp", "remap_n", "remap_stride", "remap_off", "srt_n", "srt_W", "srt_wide",
               "path", "rec_bytes", "per_partition", "wide_lb", "CH", "chunk_len")
INFO_WORDS = 24
PATH_SINGLE, PATH_TWO_LEVEL, PATH_WIDE = 0, 1, 2
Plan = namedtuple("Plan", INFO_FIELDS)


def plan_from_info(info):
    return Plan(*(int(x) for x in info[:len(INFO_FIELDS)]))


def windows_for(bits, c):
    """windows of uniform c-bit signed digits for scalars below 2^bits (one spare bit absorbs the last carry)"""
    return (bits + c) // c


def window_layout(c, W, wide):
    """-> (widths, offsets) of the W windows: c bits below `wide`, c - 1 from there on"""
    widths = [c if w < wide else c - 1 for w in range(W)]
    offs = [0] * W
    for w in range(1, W):
        offs[w] = offs[w - 1] + widths[w - 1]
    return widths, offs


def limbs_of(ints):
    """Python integers below 2^256 -> (n, 4) u64 limbs, least significant first"""
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in ints), dtype="<u8").reshape(-1, 4).astype(U64)


def signed_digits(canon, c, W, wide):
    """canon: (n, 4) u64 canonical limbs -> (W, n) int64 digits; checked against the scalars before they are returned."""
    a = np.ascontiguousarray(canon, dtype=U64).reshape(-1, 4)
    n = a.shape[0]
    widths, offs = window_layout(c, W, wide)
    assert min(widths) >= 1 and max(widths) <= 32
    limb = [a[:, k] for k in range(4)] + [np.zeros(n, dtype=U64)]
    digits = np.empty((W, n), dtype=np.int64)
    carry = np.zeros(n, dtype=np.int64)
    for w in range(W):
        cw, q, sh = widths[w], offs[w] >> 6, offs[w] & 63
        if q >= 4:
            raw = np.zeros(n, dtype=U64)
        else:
            raw = limb[q] >> U64(sh)
            if sh + cw > 64:
                raw = raw | (limb[q + 1] << U64(64 - sh))
            raw = raw & U64((1 << cw) - 1)
        v = raw.astype(np.int64) + carry
        neg = v > (1 << (cw - 1))
        digits[w] = np.where(neg, v - (1 << cw), v)
        carry = neg.astype(np.int64)
    check_digits(a, digits, widths, offs)
    return digits


def check_digits(canon, digits, widths, offs):
    """sum_w digit_w 2^(offset_w) == scalar for every scalar, and |digit_w| <= half_w. The sum is taken in 32-bit columns held in int64
    (a digit is below 2^22 in magnitude and shifted by at most 31 bits, 128 windows at most: no column passes 2^60), then normalised."""
    n = canon.shape[0]
    col = np.zeros((11, n), dtype=np.int64)
    for w in range(len(widths)):
        half = 1 << (widths[w] - 1)
        d = digits[w]
        assert int(np.abs(d).max(initial=0)) <= half, "window %d: |digit| above half" % w
        assert offs[w] >> 5 < 10
        col[offs[w] >> 5] += d << (offs[w] & 31)
    for k in range(10):
        col[k + 1] += col[k] >> 32          # floor: borrows travel as negative carries
        col[k] &= 0xffffffff
    want = np.ascontiguousarray(canon, dtype="<u8").view("<u4").reshape(n, 8).astype(np.int64)
    bad = np.nonzero((col[:8].T != want).any(axis=1) | (col[8:] != 0).any(axis=0))[0]
    assert bad.size == 0, "digits of scalar %d do not add up to it" % int(bad[0])


WindowRef = namedtuple("WindowRef", "start nlanes entries counts")


def sort_reference(canon, plan):
    """canon: (n, 4) u64 canonical scalars, plan: Plan as the harness reported it -> one WindowRef per sort window:
    start (NB + 2 u32), nlanes, entries (u32, ordered by bucket, then by value), counts (NB + 1 entries per bucket, index 0 unused)."""
    a = np.ascontiguousarray(canon, dtype=U64).reshape(-1, 4)
    n = a.shape[0]
    digits = signed_digits(a, plan.c, plan.W, plan.wide)
    Wp = plan.srt_W
    rows = plan.srt_n // n                                     # table rows; 1 for plain plans (a row past the last window stays empty)
    assert plan.srt_n == n * rows and rows * Wp >= plan.W and (plan.remap_n == n or (plan.remap_n == 0 and rows == 1))
    idx = np.arange(n, dtype=np.int64)
    out = []
    for ws in range(Wp):
        bucket, entry = [], []
        for k in range(rows):
            w = k * Wp + ws
            if w >= plan.W:
                continue
            d = digits[w]
            nz = d != 0
            ids = idx[nz] + (k * plan.remap_stride + plan.remap_off if plan.remap_n else 0)
            assert ids.size == 0 or int(ids.max()) < 1 << 31
            bucket.append(np.abs(d[nz]))
            entry.append((ids | ((d[nz] < 0).astype(np.int64) << 31)).astype(np.uint32))
        bucket = np.concatenate(bucket) if bucket else np.zeros(0, dtype=np.int64)
        entry = np.concatenate(entry) if entry else np.zeros(0, dtype=np.uint32)
        assert bucket.size == 0 or int(bucket.max()) <= plan.NB
        counts = np.bincount(bucket, minlength=plan.NB + 1)
        start = np.zeros(plan.NB + 2, dtype=np.int64)
        start[2:] = np.cumsum(counts[1:])
        total = int(start[-1])
        lane = plan.Ln if ws >= plan.srt_wide else plan.L
        order = np.lexsort((entry, bucket))
        out.append(WindowRef(start.astype(np.uint32), -(-total // lane), entry[order], counts))
    return out


# ---- scalar sets -------------------------------------------------------------------------------------------------------------------
SET_NAMES = ("uniform", "zero", "one", "rm1", "halves", "bounds", "halfchunk", "halfchunk1", "equal", "runs", "small")


RUN_LAYOUTS = ((9, 8, 7), (7, 8, 9), (8, 8, 8, 8, 8, 9))


def wave_peels(keys):
    """What the wave-aggregated counter of the sort kernels (lds_slot, msm_sort.hpp) does with one wave: keys = the 64 lanes' bucket
    keys in lane order, 0 for a lane with nothing to count. Up to four rounds: the lowest lane still to do leads, the lanes with its
    key form its group, a group of 8 or more is peeled with one atomic, a smaller one ends the rounds (the rest: one atomic per lane).
    -> (peels, size of the group that ended the rounds or 0, largest group still to do afterwards)"""
    todo = [int(k) for k in keys if k]
    peels, stopper = 0, 0
    for _ in range(4):
        if not todo:
            break
        grp = todo.count(todo[0])
        if grp < 8:
            stopper = grp
            break
        todo = [k for k in todo if k != todo[0]]
        peels += 1
    return peels, stopper, max((todo.count(k) for k in set(todo)), default=0)


def wave_profiles(digit_row):
    """wave_peels of every full block of 64 consecutive scalars of one window's digits, as a set"""
    keys = np.abs(np.asarray(digit_row))
    return {wave_peels(keys[b:b + 64]) for b in range(0, keys.size - 63, 64)}


def chunk_scalar(r, widths, offs, plus):
    """The scalar whose chunk in every window is half_w + plus, over the windows that lie wholly below bit r.bit_length() - 1 (so the
    value is below r as it stands -- filling the top window too would need a reduction, which destroys the pattern): plus = 0 gives the
    digit +half in each of them (code 0x7FFF at c = 16), plus = 1 a negative digit in each with the carry running through all of them."""
    top = r.bit_length() - 1
    v = sum(((1 << (cw - 1)) + plus) << o for cw, o in zip(widths, offs) if o + cw <= top)
    assert v < r
    return v


def scalar_set(name, r, n, c, W, wide, seed):
    """n canonical scalars below r (Python integers) of the named set, for a plan with windows (c, W, wide)."""
    rnd = random.Random("%s/%d/%d" % (name, n, seed))     # not the layout: only the sets that follow the window boundaries depend on it
    widths, offs = window_layout(c, W, wide)
    if name == "uniform":
        return [rnd.randrange(r) for _ in range(n)]
    if name == "zero":
        return [0] * n
    if name == "one":
        return [1] * n
    if name == "rm1":
        return [r - 1] * n
    if name == "halves":
        return [((r - 1) // 2, (r + 1) // 2)[i & 1] for i in range(n)]
    if name == "bounds":                                      # 2^k and 2^k - 1 at every window boundary; reduced mod r where 2^k >= r
        vals = []
        for k in offs[1:] + [offs[-1] + widths[-1]]:
            vals += [(1 << k) % r, ((1 << k) - 1) % r]
        return [vals[i % len(vals)] for i in range(n)]
    if name == "halfchunk":
        return [chunk_scalar(r, widths, offs, 0)] * n
    if name == "halfchunk1":
        return [chunk_scalar(r, widths, offs, 1)] * n
    if name == "equal":
        return [rnd.randrange(1, r)] * n
    if name == "runs":
        # CONTIGUOUS runs of equal scalars from the first index of every block of 64 (one wave of the sort kernels wherever a chunk
        # starts at a multiple of 64), around the peel threshold of the wave-aggregated counter (8 equal keys; the leader is the lowest
        # lane still to do, so a lane between two runs would end the peeling): 9 + 8 + 7 (two peels, then the group of 7 sends the
        # rest to per-lane atomics), 7 first (no peel at all) and 8 + 8 + 8 + 8 + 8 + 9 (four peels, then the round limit with a run
        # of 8 and a run of 9 still to do). wave_peels() below says what a wave does; the tests assert that all three occur.
        out = [rnd.randrange(r) for _ in range(n)]
        for blk in range(0, n, 64):
            pos = blk
            for run in RUN_LAYOUTS[(blk // 64) % 3]:
                v = rnd.randrange(1, r)
                for i in range(pos, min(pos + run, n)):
                    out[i] = v
                pos += run
        return out
    if name == "small":
        return [rnd.randrange(256) for _ in range(n)]
    raise KeyError(name)
