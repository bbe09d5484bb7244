"""ctypes binding of include/cosnarks_hip.h (one Python function per C entry point, numpy u64 in/out).

Field elements travel as little-endian u64 limb arrays in arkworks (Montgomery) layout, exactly the bytes
a Rust ``&[Fr]`` holds -- see the header for conventions.  No arithmetic happens in this file.
"""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

BN254, BLS12_381, GRUMPKIN, BLS12_377 = 0, 1, 2, 3   # GRUMPKIN: MSM only (G1); BLS12_377: MSM (G1, G2), NTT, share vectors, reductions (no host prover mirror)
G1, G2 = 0, 1

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class CoSnarksHipError(RuntimeError):
    pass


def lib_path() -> str:
    """The in-tree build; COSNARKS_HIP_LIB points A/B runs of kernel variants at another build of the same sources."""
    return os.environ.get("COSNARKS_HIP_LIB") or os.path.join(_HERE, "lib", "libcosnarks_hip.so")


def header_path() -> str:
    return os.path.join(os.path.dirname(_HERE), "include", "cosnarks_hip.h")


def declared_symbols() -> list:
    """Every function name declared in include/cosnarks_hip.h."""
    txt = open(header_path()).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(csh_[a-z0-9_]+)\s*\(", txt)))


def lib():
    """Load the HIP library (fails loudly if it has not been built)."""
    global _LIB
    if _LIB is None:
        p = lib_path()
        if not os.path.exists(p):
            raise CoSnarksHipError(
                f"{p} not found: build it with `python co-snarks_amd/build.py` (hipcc, gfx950). "
                "There is no CPU fallback.")
        L = C.CDLL(p)
        L.csh_last_error.restype = C.c_char_p
        L.csh_version.restype = C.c_char_p
        _LIB = L
    return _LIB


def _check(rc: int):
    if rc != 0:
        raise CoSnarksHipError(f"cosnarks_hip error {rc}: {lib().csh_last_error().decode(errors='replace')}")


def device_count() -> int:
    n = C.c_int(0)
    rc = lib().csh_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def have_device() -> bool:
    try:
        return device_count() > 0
    except CoSnarksHipError:
        return False


def fr_bytes(curve: int) -> int:
    return 32


def fq_bytes(curve: int) -> int:
    return 48 if curve in (BLS12_381, BLS12_377) else 32


def point_bytes(curve: int, group: int) -> int:
    return 2 * fq_bytes(curve) * (2 if group == G2 else 1)


def _u64(a, copy=False):
    arr = np.ascontiguousarray(a, dtype=np.uint64)
    return arr.copy() if copy and arr is a else arr


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class DeviceBuffer:
    """Raw device allocation through the C ABI (csh_malloc / csh_memcpy_*)."""

    def __init__(self, nbytes: int):
        self.nbytes = int(nbytes)
        self.ptr = C.c_void_p()
        _check(lib().csh_malloc(C.byref(self.ptr), C.c_size_t(self.nbytes)))

    @classmethod
    def from_host(cls, arr):
        a = np.ascontiguousarray(arr)
        b = cls(a.nbytes)
        _check(lib().csh_memcpy_h2d(b.ptr, _p(a), C.c_size_t(a.nbytes)))
        return b

    def to_host(self, dtype=np.uint64, count=None):
        n = self.nbytes // np.dtype(dtype).itemsize if count is None else count
        out = np.empty(n, dtype=dtype)
        _check(lib().csh_memcpy_d2h(_p(out), self.ptr, C.c_size_t(out.nbytes)))
        return out

    def free(self):
        if self.ptr:
            lib().csh_free(self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _devptr(x):
    if isinstance(x, DeviceBuffer):
        return x.ptr
    if x is None:
        return None
    if isinstance(x, C.c_void_p):
        return x
    return C.c_void_p(int(x))  # raw address, e.g. torch.Tensor.data_ptr()


def _stream(s):
    return C.c_void_p(int(s)) if s else None


class Bases:
    """Device-resident MSM bases (a proving-key query): csh_bases_upload / csh_msm."""

    def __init__(self, curve: int, group: int, points, stride_bytes: int = 0):
        self.curve, self.group = curve, group
        pts = _u64(points)
        pb = point_bytes(curve, group)
        stride = stride_bytes or pb
        assert pts.nbytes % stride == 0
        self.n = pts.nbytes // stride
        self.h = C.c_void_p()
        _check(lib().csh_bases_upload(curve, group, _p(pts), C.c_size_t(self.n), C.c_size_t(stride_bytes), C.byref(self.h)))

    def _out(self):
        return np.zeros(3 * point_bytes(self.curve, self.group) // 2 // 8, dtype=np.uint64)

    def precompute(self, c: int = 0, groups: int = 0):
        """csh_bases_precompute[_grouped]: fixed-base tables (merged-window MSMs on this handle); groups = 0: one row per window."""
        if groups:
            _check(lib().csh_bases_precompute_grouped(self.h, int(c), int(groups)))
        else:
            _check(lib().csh_bases_precompute(self.h, int(c)))
        return self

    def msm(self, scalars, offset: int = 0, n: int | None = None, montgomery: bool = True):
        """-> Jacobian (X, Y, Z) limbs (Z in {0, 1}). scalars: (n, 4) u64 host array."""
        sc = _u64(scalars)
        cnt = sc.size // 4 if n is None else n
        out = self._out()
        _check(lib().csh_msm(self.h, C.c_size_t(offset), C.c_size_t(cnt), _p(sc), int(montgomery), _p(out)))
        return out

    def msm_dev(self, scalars_dev, n: int, offset: int = 0, montgomery: bool = True, stream=None):
        out = self._out()
        _check(lib().csh_msm_dev(self.h, C.c_size_t(offset), C.c_size_t(n), _devptr(scalars_dev), int(montgomery), _p(out), _stream(stream)))
        return out

    def msm_partial_dev(self, scalars_dev, n: int, out_dev, offset: int = 0, montgomery: bool = True, stream=None):
        _check(lib().csh_msm_partial_dev(self.h, C.c_size_t(offset), C.c_size_t(n), _devptr(scalars_dev), int(montgomery),
                                         _devptr(out_dev), _stream(stream)))

    def free(self):
        if self.h:
            lib().csh_bases_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def msm_partial_bytes(curve: int, group: int) -> int:
    n = C.c_size_t(0)
    _check(lib().csh_msm_partial_bytes(curve, group, C.byref(n)))
    return n.value


def msm_fold_partials(curve: int, group: int, partials: np.ndarray, nparts: int):
    buf = np.ascontiguousarray(partials)
    out = np.zeros(3 * point_bytes(curve, group) // 2 // 8, dtype=np.uint64)
    _check(lib().csh_msm_fold_partials(curve, group, _p(buf), C.c_size_t(nparts), _p(out)))
    return out


def msm_plan(curve: int, n: int):
    """csh_msm_plan: (c, W, L, S, accumulate waves, SIMDs) an n-point MSM would run with; host-only."""
    out = (C.c_uint32 * 6)()
    _check(lib().csh_msm_plan(curve, C.c_size_t(n), out))
    return tuple(int(x) for x in out)


def tune_set(key: str, value: int):
    """csh_tune_set: process-wide tuning knob (tests / A-B runs)."""
    _check(lib().csh_tune_set(key.encode(), int(value)))


def tune_get(key: str) -> int:
    v = C.c_int(0)
    _check(lib().csh_tune_get(key.encode(), C.byref(v)))
    return v.value


class tuned:
    """with tuned(msm_c=11, sort_two_level=1): ...  -- sets knobs, restores the previous values on exit."""

    def __init__(self, **kv):
        self.kv = kv
        self.old = {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.old[k] = tune_get(k)
            tune_set(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            tune_set(k, v)
        return False


SPLIT_PEER, SPLIT_HOST, SPLIT_RCCL = 0, 1, 2
COMM_ID_BYTES = 128


def comm_unique_id() -> bytes:
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    _check(lib().csh_comm_unique_id(buf))
    return bytes(buf)


class Comm:
    """csh_comm_t: one rank of a split-MSM communicator (RCCL behind the C ABI; no torch)."""

    def __init__(self, handle):
        self.h = handle

    @classmethod
    def init_rank(cls, uid, nranks: int, rank: int):
        h = C.c_void_p()
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(uid) if uid is not None else None
        _check(lib().csh_comm_init_rank(buf, int(nranks), int(rank), C.byref(h)))
        return cls(h)

    @classmethod
    def init_all(cls, devices):
        k = len(devices)
        arr = (C.c_int * k)(*devices)
        hs = (C.c_void_p * k)()
        _check(lib().csh_comm_init_all(arr, k, hs))
        return [cls(C.c_void_p(hs[i])) for i in range(k)]

    def info(self):
        r, n, d = C.c_int(0), C.c_int(0), C.c_int(0)
        _check(lib().csh_comm_info(self.h, C.byref(r), C.byref(n), C.byref(d)))
        return r.value, n.value, d.value

    def msm_split_rank_dev(self, bases: "Bases", scalars_dev, n: int, offset: int = 0, montgomery: bool = True, stream=None):
        out = bases._out()
        _check(lib().csh_msm_split_rank_dev(self.h, bases.h, C.c_size_t(offset), C.c_size_t(n), _devptr(scalars_dev), int(montgomery),
                                            _p(out), _stream(stream)))
        return out

    def destroy(self):
        if self.h:
            lib().csh_comm_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def msm_split(bases, offsets, counts, scalars_dev, montgomery: bool = True, mode: int = SPLIT_PEER, comms=None):
    """csh_msm_split: one MSM over k ranges (one thread drives every device). bases: list of Bases; scalars_dev: list of
    device pointers / DeviceBuffers."""
    k = len(bases)
    hs = (C.c_void_p * k)(*[b.h.value for b in bases])
    offs = (C.c_size_t * k)(*offsets)
    cnts = (C.c_size_t * k)(*counts)
    ptrs = (C.c_void_p * k)(*[(_devptr(s).value if s is not None else None) for s in scalars_dev])
    cm = (C.c_void_p * k)(*[c.h.value for c in comms]) if comms else None
    out = bases[0]._out()
    _check(lib().csh_msm_split(hs, offs, cnts, ptrs, C.c_size_t(k), int(montgomery), int(mode), cm, _p(out)))
    return out


def msm_last_timing():
    out = (C.c_float * 6)()
    _check(lib().csh_msm_last_timing(out))
    return list(out)


def msm_last_params():
    """[window bits c, windows W, entries per lane L, reduction segments S] of the last MSM on this thread."""
    out = (C.c_uint32 * 4)()
    _check(lib().csh_msm_last_params(out))
    return list(out)


class Domain:
    """taceo_ark_algebra::fft::Domain equivalent: csh_domain_create + transforms."""

    def __init__(self, curve: int, log_n: int, group_gen=None):
        self.curve, self.log_n, self.n = curve, log_n, 1 << log_n
        self.h = C.c_void_p()
        gg = _u64(group_gen) if group_gen is not None else None
        _check(lib().csh_domain_create(curve, C.c_uint32(log_n), _p(gg), C.byref(self.h)))

    def _host(self, fn, data, ncomp):
        d = _u64(data).copy()
        assert d.size == self.n * ncomp * 4, (d.size, self.n, ncomp)
        _check(fn(self.h, _p(d), C.c_uint32(ncomp)))
        return d

    def ifft_in_to_out(self, data, ncomp=1):
        return self._host(lib().csh_ifft_in_to_out, data, ncomp)

    def fft_out_to_in(self, data, ncomp=1):
        return self._host(lib().csh_fft_out_to_in, data, ncomp)

    def fft(self, data, ncomp=1):
        return self._host(lib().csh_fft, data, ncomp)

    def ifft(self, data, ncomp=1):
        return self._host(lib().csh_ifft, data, ncomp)

    def coset_table(self, shift):
        out = np.zeros(self.n * 4, dtype=np.uint64)
        sh = _u64(shift)
        _check(lib().csh_coset_table(self.h, _p(sh), _p(out)))
        return out

    # device-pointer variants (asynchronous on `stream`)
    def ifft_in_to_out_dev(self, data_dev, ncomp=1, stream=None):
        _check(lib().csh_ifft_in_to_out_dev(self.h, _devptr(data_dev), C.c_uint32(ncomp), _stream(stream)))

    def fft_out_to_in_dev(self, data_dev, ncomp=1, stream=None):
        _check(lib().csh_fft_out_to_in_dev(self.h, _devptr(data_dev), C.c_uint32(ncomp), _stream(stream)))

    def fft_dev(self, data_dev, ncomp=1, stream=None):
        _check(lib().csh_fft_dev(self.h, _devptr(data_dev), C.c_uint32(ncomp), _stream(stream)))

    def ifft_dev(self, data_dev, ncomp=1, stream=None):
        _check(lib().csh_ifft_dev(self.h, _devptr(data_dev), C.c_uint32(ncomp), _stream(stream)))

    def free(self):
        if self.h:
            lib().csh_domain_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def bit_reverse(curve: int, data, log_n: int, ncomp: int = 1):
    d = _u64(data).copy()
    _check(lib().csh_bit_reverse(curve, _p(d), C.c_uint32(log_n), C.c_uint32(ncomp)))
    return d


def vec_mul(curve: int, a, b):
    a, b = _u64(a), _u64(b)
    out = np.empty_like(a)
    _check(lib().csh_vec_mul(curve, _p(a), _p(b), _p(out), C.c_size_t(a.size // 4)))
    return out


def vec_add(curve: int, a, b, ncomp: int = 1):
    a, b = _u64(a), _u64(b)
    out = np.empty_like(a)
    _check(lib().csh_vec_add(curve, _p(a), _p(b), _p(out), C.c_size_t(a.size // (4 * ncomp)), C.c_uint32(ncomp)))
    return out


def vec_sub(curve: int, a, b, ncomp: int = 1):
    a, b = _u64(a), _u64(b)
    out = np.empty_like(a)
    _check(lib().csh_vec_sub(curve, _p(a), _p(b), _p(out), C.c_size_t(a.size // (4 * ncomp)), C.c_uint32(ncomp)))
    return out


def vec_mul_table(curve: int, v, table, ncomp: int = 1):
    v = _u64(v).copy()
    t = _u64(table)
    _check(lib().csh_vec_mul_table(curve, _p(v), _p(t), C.c_size_t(t.size // 4), C.c_uint32(ncomp)))
    return v


def vec_prefix_prod(curve: int, v, n: int | None = None, out=None, stream=None):
    """csh_vec_prefix_prod: out[i] = v[0] * ... * v[i]. A host array gives a host array; a DeviceBuffer (with n) runs the stream-ordered
    form into `out` (default: in place) and returns that buffer."""
    if isinstance(v, DeviceBuffer):
        out = v if out is None else out
        _check(lib().csh_vec_prefix_prod_dev(curve, _devptr(v), _devptr(out), C.c_size_t(n), _stream(stream)))
        return out
    a = _u64(v)
    res = np.empty_like(a)
    _check(lib().csh_vec_prefix_prod(curve, _p(a), _p(res), C.c_size_t(a.size // 4)))
    return res


def vec_batch_inverse(curve: int, v, n: int | None = None, out=None, zero_count=None, stream=None):
    """csh_vec_batch_inverse: -> (out, zero_count); out[i] = v[i]^-1, zeros stay zero. Host array: host results. DeviceBuffer (with n):
    the stream-ordered form into `out` (default: in place); zero_count = an 8-byte DeviceBuffer for the count, or None (NULL),
    handed back as given."""
    if isinstance(v, DeviceBuffer):
        out = v if out is None else out
        _check(lib().csh_vec_batch_inverse_dev(curve, _devptr(v), _devptr(out), C.c_size_t(n), _devptr(zero_count), _stream(stream)))
        return out, zero_count
    a = _u64(v)
    res = np.empty_like(a)
    zc = C.c_size_t(0)
    _check(lib().csh_vec_batch_inverse(curve, _p(a), _p(res), C.c_size_t(a.size // 4), C.byref(zc)))
    return res, zc.value


def eval_poly(curve: int, coeffs, point, ncomp: int = 1, n: int | None = None, out=None, stream=None):
    """csh_eval_poly: sum_i coeffs[i] point^i per share component -> ncomp field elements. `point` is a host element (4 limbs).
    DeviceBuffer coefficients (with n): the stream-ordered form into the DeviceBuffer `out` (32 * ncomp bytes), which is returned."""
    pt = _u64(point)
    assert pt.size == 4
    if isinstance(coeffs, DeviceBuffer):
        out = DeviceBuffer(32 * ncomp) if out is None else out
        _check(lib().csh_eval_poly_dev(curve, _devptr(coeffs), C.c_size_t(n), C.c_uint32(ncomp), _p(pt), _devptr(out), _stream(stream)))
        return out
    a = _u64(coeffs)
    res = np.empty(4 * ncomp, dtype=np.uint64)
    _check(lib().csh_eval_poly(curve, _p(a) if a.size else None, C.c_size_t(a.size // (4 * ncomp)), C.c_uint32(ncomp), _p(pt), _p(res)))
    return res


def poly_div_linear(curve: int, coeffs, root, ncomp: int = 1, sub0=None, n: int | None = None, out=None, rem=None, scale=None,
                    accumulate: bool = False, stream=None):
    """csh_poly_div_linear: division by (X - root) in the reference's direction, b_i = (-root)^-1 (coeffs[i] - b_(i-1)) -> (quotient
    b_0 .. b_(n-2), rem = b_(n-1), ncomp elements: 0 exactly when the division is exact). `root`, `sub0` (ncomp elements taken off
    coefficient 0 as it is loaded) and `scale` are host elements. A host array gives host arrays. DeviceBuffer coefficients (with n): the
    stream-ordered form; out (default: in place) receives scale * b, or with accumulate has it added to what it holds (out must then be
    another buffer); rem = a DeviceBuffer of 32 * ncomp bytes or None (NULL). Returns (out, rem) as given."""
    rt = _u64(root)
    assert rt.size == 4
    s0 = _u64(sub0) if sub0 is not None else None
    assert s0 is None or s0.size == 4 * ncomp
    if isinstance(coeffs, DeviceBuffer):
        out = coeffs if out is None else out
        sc = _u64(scale) if scale is not None else None
        assert sc is None or sc.size == 4
        _check(lib().csh_poly_div_linear_dev(curve, _devptr(coeffs), C.c_size_t(n), C.c_uint32(ncomp), _p(rt), _p(s0), _p(sc), int(bool(accumulate)),
                                             _devptr(out), _devptr(rem), _stream(stream)))
        return out, rem
    assert scale is None and not accumulate, "scale / accumulate: the device form only"
    a = _u64(coeffs)
    cnt = a.size // (4 * ncomp)
    res = np.empty(4 * ncomp * max(cnt - 1, 0), dtype=np.uint64)
    r = np.empty(4 * ncomp, dtype=np.uint64)
    _check(lib().csh_poly_div_linear(curve, _p(a) if a.size else None, C.c_size_t(cnt), C.c_uint32(ncomp), _p(rt), _p(s0), _p(res) if res.size else None, _p(r)))
    return res, r


def mle_fold(curve: int, vecs, u, ncomp: int = 1, n: int | None = None, outs=None, stream=None):
    """csh_mle_fold: one multilinear fold round on k vectors, out[v][j] = in[v][2j] + u (in[v][2j+1] - in[v][2j]). `u` is a host element.
    A list of host arrays gives a list of host arrays. A list of DeviceBuffers (with n): the stream-ordered form into the DeviceBuffers
    `outs` (n / 2 elements each, never one of the inputs), which are returned."""
    uu = _u64(u)
    assert uu.size == 4
    k = len(vecs)
    if k and isinstance(vecs[0], DeviceBuffer):
        ins = (C.c_void_p * k)(*[_devptr(v).value for v in vecs])
        ous = (C.c_void_p * k)(*[_devptr(o).value for o in outs])
        _check(lib().csh_mle_fold_dev(curve, ins, ous, C.c_size_t(k), C.c_size_t(n), C.c_uint32(ncomp), _p(uu), _stream(stream)))
        return outs
    arrs = [_u64(v) for v in vecs]
    cnt = arrs[0].size // (4 * ncomp) if k else 0
    res = [np.empty(4 * ncomp * (cnt // 2), dtype=np.uint64) for _ in arrs]
    ins = (C.c_void_p * k)(*[a.ctypes.data for a in arrs])
    ous = (C.c_void_p * k)(*[r.ctypes.data for r in res])
    _check(lib().csh_mle_fold(curve, ins, ous, C.c_size_t(k), C.c_size_t(cnt), C.c_uint32(ncomp), _p(uu)))
    return res


def mle_fold_rounds(curve: int, vec, us, ncomp: int = 1, n: int | None = None, levels=True, last=True, stream=None):
    """csh_mle_fold_rounds: m = len(us) / 4 fold rounds on one vector -> (levels, last). levels: levels 1..m back to back (level l at
    element offset n - n / 2^(l-1)), last: level m alone; with n = 2^m that is the value of evaluate_mle. Host array: `levels` / `last`
    are flags, host arrays (or None) come back. DeviceBuffer (with n): they are DeviceBuffers or None, handed back as given."""
    uu = _u64(us)
    m = uu.size // 4
    if isinstance(vec, DeviceBuffer):
        lv = levels if isinstance(levels, DeviceBuffer) else None
        la = last if isinstance(last, DeviceBuffer) else None
        _check(lib().csh_mle_fold_rounds_dev(curve, _devptr(vec), C.c_size_t(n), C.c_uint32(ncomp), _p(uu), C.c_size_t(m), _devptr(lv), _devptr(la),
                                             _stream(stream)))
        return lv, la
    a = _u64(vec)
    cnt = a.size // (4 * ncomp)
    lv = np.empty(4 * ncomp * (cnt - (cnt >> m)), dtype=np.uint64) if levels else None
    la = np.empty(4 * ncomp * (cnt >> m), dtype=np.uint64) if last else None
    _check(lib().csh_mle_fold_rounds(curve, _p(a), C.c_size_t(cnt), C.c_uint32(ncomp), _p(uu), C.c_size_t(m), _p(lv), _p(la)))
    return lv, la


def _devptr_array(bufs):
    return (C.c_void_p * len(bufs))(*[_devptr(b).value if b is not None else None for b in bufs]) if len(bufs) else None


def plonk_quot_blinders(dom: "Domain", protocol: int, party: int, blinders, outs, stream=None):
    """csh_plonk_quot_blinders_dev: stage (a) of the PLONK quotient on the extended domain `dom`. blinders: the host shares b0..b8;
    outs: the DeviceBuffers ap, bp, cp, zp, zwp (N ncomp elements each), which are returned."""
    b = _u64(blinders)
    assert b.size == 9 * 4 * (protocol + 1) and len(outs) == 5
    _check(lib().csh_plonk_quot_blinders_dev(dom.h, C.c_uint32(protocol), C.c_uint32(party), _p(b), _devptr_array(outs), _stream(stream)))
    return outs


def plonk_quot_operands(dom: "Domain", protocol: int, party: int, shares, public, lagrange, buffer_a, challenges, outs, stream=None):
    """csh_plonk_quot_operands_dev: stage (b). shares: the 11 DeviceBuffers a, b, c, z, a_b, a_bp, ap_b, ap_bp, ap, bp, cp; public: the 8
    DeviceBuffers qm, ql, qr, qo, qc, s1, s2, s3; lagrange: the n_public DeviceBuffers L_1..L_np; buffer_a: the n_public host shares;
    challenges: beta, gamma, k1, k2 on the host; outs: the 10 DeviceBuffers pi, e1, e1z, e2a, e2b, e2c, e3a, e3b, e3c, e3d, which are returned."""
    ba, ch = _u64(buffer_a), _u64(challenges)
    npub = len(lagrange)
    assert len(shares) == 11 and len(public) == 8 and len(outs) == 10 and ch.size == 16 and ba.size == npub * 4 * (protocol + 1)
    _check(lib().csh_plonk_quot_operands_dev(dom.h, C.c_uint32(protocol), C.c_uint32(party), _devptr_array(shares), _devptr_array(public),
                                             _devptr_array(lagrange), C.c_size_t(npub), _p(ba) if npub else None, _p(ch), _devptr_array(outs),
                                             _stream(stream)))
    return outs


def plonk_quot_combine(dom: "Domain", protocol: int, party: int, shares, lagrange1, alpha, outs, stream=None):
    """csh_plonk_quot_combine_dev: stage (c). shares: the 14 DeviceBuffers e1, e1z, z, zp, e2, e2z_0..3, e3, e3z_0..3; lagrange1: L_1;
    alpha on the host; outs: the DeviceBuffers t, tz, which are returned."""
    al = _u64(alpha)
    assert len(shares) == 14 and len(outs) == 2 and al.size == 4
    _check(lib().csh_plonk_quot_combine_dev(dom.h, C.c_uint32(protocol), C.c_uint32(party), _devptr_array(shares), _devptr(lagrange1), _p(al),
                                            _devptr_array(outs), _stream(stream)))
    return outs


def plonk_quot_finish(curve: int, n: int, protocol: int, party: int, ct, ctz, b9_b10, t1, t2, t3, stream=None):
    """csh_plonk_quot_finish_dev: stage (d) on the coefficient forms ct, ctz (4 n shares each) -> the DeviceBuffers t1, t2 (n + 1 shares)
    and t3 (n + 6 shares), which are returned."""
    bb = _u64(b9_b10)
    assert bb.size == 2 * 4 * (protocol + 1)
    _check(lib().csh_plonk_quot_finish_dev(curve, C.c_size_t(n), C.c_uint32(protocol), C.c_uint32(party), _devptr(ct), _devptr(ctz), _p(bb),
                                           _devptr(t1), _devptr(t2), _devptr(t3), _stream(stream)))
    return t1, t2, t3


def plonk_z_operands(dom: "Domain", protocol: int, party: int, shares, sigma, challenges, outs, stream=None):
    """csh_plonk_z_operands_dev on the EXTENDED domain `dom` (4 n points). shares: the DeviceBuffers buffer_a, buffer_b, buffer_c (n shares);
    sigma: the DeviceBuffers S1, S2, S3 (4 n evaluations); challenges: beta, gamma, k1, k2 on the host; outs: the 6 DeviceBuffers n1, n2, n3,
    d1, d2, d3, which are returned."""
    ch = _u64(challenges)
    assert len(shares) == 3 and len(sigma) == 3 and len(outs) == 6 and ch.size == 16
    _check(lib().csh_plonk_z_operands_dev(dom.h, C.c_uint32(protocol), C.c_uint32(party), _devptr_array(shares), _devptr_array(sigma), _p(ch),
                                          _devptr_array(outs), _stream(stream)))
    return outs


def vec_rotate_right(curve: int, vec, out, n: int, ncomp: int = 1, k: int = 1, stream=None):
    """csh_vec_rotate_right_dev: out[(i + k) mod n] = vec[i] on DeviceBuffers of n shares; out is returned."""
    _check(lib().csh_vec_rotate_right_dev(curve, _devptr(vec), _devptr(out), C.c_size_t(n), C.c_uint32(ncomp), C.c_size_t(k), _stream(stream)))
    return out


def plonk_blind_coefficients(curve: int, poly, n: int, coeff_rev, ncomp: int = 1, stream=None):
    """csh_plonk_blind_coefficients_dev: poly (a DeviceBuffer with room for n + k shares) in place; coeff_rev: the k host shares."""
    cr = _u64(coeff_rev)
    k = cr.size // (4 * ncomp)
    assert cr.size == k * 4 * ncomp
    _check(lib().csh_plonk_blind_coefficients_dev(curve, _devptr(poly), C.c_size_t(n), C.c_uint32(ncomp), _p(cr), C.c_size_t(k), _stream(stream)))
    return poly


def poly_lincomb(curve: int, protocol: int, party: int, shares, share_lens, share_coeffs, public, public_lens, public_coeffs, out, out_len: int,
                 const0=None, stream=None):
    """csh_poly_lincomb_dev: out[i] = sum cs_j S_j[i] (+) (sum cp_j P_j[i] + [i = 0] const0) over DeviceBuffers of differing lengths
    (share_lens in shares, public_lens in elements); the coefficients and const0 are host elements. out (out_len shares) is returned."""
    cs, cp = _u64(share_coeffs), _u64(public_coeffs)
    ks, kp = len(shares), len(public)
    assert cs.size == 4 * ks and cp.size == 4 * kp and len(share_lens) == ks and len(public_lens) == kp
    c0 = _u64(const0) if const0 is not None else None
    sl, pl = (C.c_size_t * ks)(*share_lens), (C.c_size_t * kp)(*public_lens)
    _check(lib().csh_poly_lincomb_dev(curve, C.c_uint32(protocol), C.c_uint32(party), _devptr_array(shares), sl if ks else None, _p(cs) if ks else None,
                                      C.c_size_t(ks), _devptr_array(public), pl if kp else None, _p(cp) if kp else None, C.c_size_t(kp), _p(c0),
                                      _devptr(out), C.c_size_t(out_len), _stream(stream)))
    return out


class HonkMemoryRecords:
    """The memory-record rows of an UltraHonk proving key (memory_read_records, memory_write_records and the rows of
    memory_records_shared) as uint32 lists on the device, uploaded once. The contract of csh_honk_w4_records_dev is checked here, on the
    host: every index is below n and occurs once, within a list or across lists."""

    def __init__(self, n: int, read=(), write=(), shared=()):
        lists = [np.ascontiguousarray(np.asarray(v, dtype=np.int64).reshape(-1)) for v in (read, write, shared)]
        every = np.concatenate(lists)
        if every.size and (every.min() < 0 or every.max() >= n):
            raise CoSnarksHipError("honk memory records: an index is outside 0 .. n - 1")
        if np.unique(every).size != every.size:
            raise CoSnarksHipError("honk memory records: an index occurs twice (a duplicate would be a race on the device)")
        self.n = int(n)
        self.counts = [int(v.size) for v in lists]
        self.bufs = [DeviceBuffer.from_host(v.astype(np.uint32)) if v.size else None for v in lists]


def honk_w4_records(curve: int, protocol: int, party: int, w, w4, n: int, etas, records: "HonkMemoryRecords", type_share=None, stream=None):
    """csh_honk_w4_records_dev: w = the DeviceBuffers w_l, w_r, w_o (n shares); w4 (n shares) in place, returned; etas = eta_1, eta_2,
    eta_3 on the host; type_share = the DeviceBuffer of the shared records' type shares (None without shared records)."""
    et = _u64(etas)
    assert len(w) == 3 and et.size == 12 and records.n == n
    nr, nw, ns = records.counts
    _check(lib().csh_honk_w4_records_dev(curve, C.c_uint32(protocol), C.c_uint32(party), _devptr_array(w), _devptr(w4), C.c_size_t(n), _p(et),
                                         _devptr(records.bufs[0]), C.c_size_t(nr), _devptr(records.bufs[1]), C.c_size_t(nw),
                                         _devptr(records.bufs[2]), _devptr(type_share), C.c_size_t(ns), _stream(stream)))
    return w4


def honk_lookup_operands(curve: int, protocol: int, party: int, shares, public, n: int, challenges, outs, stream=None):
    """csh_honk_lookup_operands_dev: shares = the DeviceBuffers w_l, w_r, w_o, lookup_read_tags (n shares); public = q_r, q_m, q_c, q_o,
    table_1..4, q_lookup (n elements); challenges = beta, gamma on the host; outs = the DeviceBuffers prod, sel, which are returned."""
    ch = _u64(challenges)
    assert len(shares) == 4 and len(public) == 9 and len(outs) == 2 and ch.size == 8
    _check(lib().csh_honk_lookup_operands_dev(curve, C.c_uint32(protocol), C.c_uint32(party), _devptr_array(shares), _devptr_array(public),
                                              C.c_size_t(n), _p(ch), _devptr_array(outs), _stream(stream)))
    return outs


def _honk_ranges(ranges):
    flat = [int(x) for r in (ranges or ()) for x in r]
    return ((C.c_size_t * len(flat))(*flat) if flat else None), len(flat) // 2


def honk_perm_operands(curve: int, protocol: int, party: int, shares, public, n: int, domain_size: int, ranges, challenges, outs, stream=None):
    """csh_honk_perm_operands_dev: shares = the DeviceBuffers w_l, w_r, w_o, w_4 (n shares); public = id_1..4, sigma_1..4 (n elements);
    ranges = the active ranges [(start, end), ...] or None; challenges = beta, gamma on the host; outs = the DeviceBuffers n_1..4, d_1..4
    (m shares each), which are returned."""
    ch = _u64(challenges)
    assert len(shares) == 4 and len(public) == 8 and len(outs) == 8 and ch.size == 8
    rg, nr = _honk_ranges(ranges)
    _check(lib().csh_honk_perm_operands_dev(curve, C.c_uint32(protocol), C.c_uint32(party), _devptr_array(shares), _devptr_array(public),
                                            C.c_size_t(n), C.c_size_t(domain_size), rg, C.c_size_t(nr), _p(ch), _devptr_array(outs),
                                            _stream(stream)))
    return outs


def honk_z_perm_place(curve: int, protocol: int, party: int, mul, z, n: int, domain_size: int, ranges, stream=None):
    """csh_honk_z_perm_place_dev: mul (m shares) -> every element of z (n shares), which is returned; ranges as honk_perm_operands."""
    rg, nr = _honk_ranges(ranges)
    _check(lib().csh_honk_z_perm_place_dev(curve, C.c_uint32(protocol), C.c_uint32(party), _devptr(mul), _devptr(z), C.c_size_t(n),
                                           C.c_size_t(domain_size), rg, C.c_size_t(nr), _stream(stream)))
    return z


HONK_SUMCHECK_COLUMNS = 36        # witness (8), shifted witness (5), precomputed (23): the order of include/cosnarks_hip.h
HONK_SUMCHECK_PARAMS = 3          # beta, gamma, public_input_delta
HONK_SUMCHECK_ACC_ELEMS = 57      # 6 + 5 + 6 + 3 + 5 + 5 + 3 + 6 + 6 + 6 + 6
HONK_GATES_COLUMNS = 19           # w (4), shifted w (4), q_m .. q_4 (6), the five gate selectors: the order of include/cosnarks_hip.h
HONK_GATES_PARAMS = 8             # eta_1..3, curve_b, mat_internal_diag_m_1[0..4)
HONK_GATES_ACC_ELEMS = 110        # 2 * 6 + 6 * 6 + 6 + 4 * 7 + 4 * 7
HONK_MAX_EDGE_END = 1 << 28


def _honk_accumulate(what, ncols, nparams, acc_elems, curve, cols, edge_begin, edge_end, params, acc, scaling, scaling_stride, stream):
    """The plain round's two entries: csh_<what>_dev after the column count, the parameter count and the range rules."""
    if len(cols) != ncols:
        raise CoSnarksHipError("%s: %d columns, not %d" % (what, len(cols), ncols))
    if edge_begin < 0 or edge_begin % 2 or edge_end % 2 or not edge_begin < edge_end <= HONK_MAX_EDGE_END:
        raise CoSnarksHipError("%s: edge_begin and edge_end must be even, edge_begin < edge_end <= 2^28" % what)
    if scaling is not None and not 1 <= scaling_stride <= HONK_MAX_EDGE_END:
        raise CoSnarksHipError("%s: scaling_stride must be 1 .. 2^28" % what)
    pr = _u64(params)
    if pr.size != 4 * nparams:
        raise CoSnarksHipError("%s: %d parameter words, not %d elements of 4" % (what, pr.size, nparams))
    if acc is None:
        acc = DeviceBuffer(32 * acc_elems)
    _check(getattr(lib(), "csh_%s_dev" % what)(curve, _devptr_array(cols), C.c_size_t(edge_begin), C.c_size_t(edge_end), _devptr(scaling),
                                               C.c_size_t(scaling_stride), _p(pr), _devptr(acc), _stream(stream)))
    return acc


def honk_sumcheck_accumulate(curve: int, cols, edge_begin: int, edge_end: int, params, acc=None, scaling=None, scaling_stride: int = 1, stream=None):
    """csh_honk_sumcheck_accumulate_dev: cols = the 36 DeviceBuffers (or device addresses) in the header's order; elements
    [edge_begin, edge_end) of each are read; params = beta, gamma, public_input_delta on the host; scaling = the DeviceBuffer of the
    gate-separator products (honk_pow_table) read at (e >> 1) * scaling_stride, or None for the factor one. acc (57 elements, made here
    unless given) is returned. The column count, the parameter count and the range rules are checked here, before the call."""
    return _honk_accumulate("honk_sumcheck_accumulate", HONK_SUMCHECK_COLUMNS, HONK_SUMCHECK_PARAMS, HONK_SUMCHECK_ACC_ELEMS, curve, cols,
                            edge_begin, edge_end, params, acc, scaling, scaling_stride, stream)


def honk_sumcheck_accumulate_gates(curve: int, cols, edge_begin: int, edge_end: int, params, acc=None, scaling=None, scaling_stride: int = 1,
                                   stream=None):
    """csh_honk_sumcheck_accumulate_gates_dev: cols = the 19 DeviceBuffers (or device addresses) in the header's order; params = eta_1,
    eta_2, eta_3, curve_b and the four internal diagonal values on the host (8 elements); range and scaling as honk_sumcheck_accumulate.
    acc (110 elements, made here unless given) is returned. The column count, the parameter count and the range rules are checked here,
    before the call."""
    return _honk_accumulate("honk_sumcheck_accumulate_gates", HONK_GATES_COLUMNS, HONK_GATES_PARAMS, HONK_GATES_ACC_ELEMS, curve, cols,
                            edge_begin, edge_end, params, acc, scaling, scaling_stride, stream)


def honk_pow_table(curve: int, betas, out=None, stream=None):
    """csh_honk_pow_table_dev: betas = m host elements, 0 <= m <= 28 -> the DeviceBuffer of the 2^m products (made here unless given)."""
    b = _u64(betas) if betas is not None and len(betas) else None
    m = 0 if b is None else b.size // 4
    if (b is not None and b.size != 4 * m) or m > 28:
        raise CoSnarksHipError("honk_pow_table: m must be 0 .. 28 elements of 4 words")
    if out is None:
        out = DeviceBuffer(32 << m)
    _check(lib().csh_honk_pow_table_dev(curve, _p(b), C.c_size_t(m), _devptr(out), _stream(stream)))
    return out


# ---- the sumcheck round on shares (csrc/honk_co_relations.hip): one wrapper per entry of include/cosnarks_hip.h ----------------------
HONK_CO_POINTS = 7                # batch elements per kept edge


class HonkCoBatch:
    """What the stages of one relation's batch share: the party, the 36 columns (DeviceBuffers, device addresses, or None for a column
    the stage does not read), the range, the kept edges (edge_idx = the DeviceBuffer of honk_co_select_edges with m = its count, or None
    for every edge of the range), the scaling table and the host parameters beta, gamma, public_input_delta. The column count and the
    range rules are checked here, before any call."""
    COLUMNS = HONK_SUMCHECK_COLUMNS
    PARAMS = (3, "beta, gamma, public_input_delta")

    def __init__(self, curve: int, protocol: int, party: int, cols, edge_begin: int, edge_end: int, edge_idx=None, m=None, scaling=None,
                 scaling_stride: int = 1, params=None):
        if len(cols) != self.COLUMNS:
            raise CoSnarksHipError("honk_co: %d columns, not %d" % (len(cols), self.COLUMNS))
        if protocol not in (0, 1) or party not in (0, 1, 2):
            raise CoSnarksHipError("honk_co: protocol must be 0 (plain / Shamir) or 1 (Rep3), party 0, 1 or 2")
        if edge_begin < 0 or edge_begin % 2 or edge_end % 2 or not edge_begin < edge_end <= HONK_MAX_EDGE_END:
            raise CoSnarksHipError("honk_co: edge_begin and edge_end must be even, edge_begin < edge_end <= 2^28")
        if scaling is not None and not 1 <= scaling_stride <= HONK_MAX_EDGE_END:
            raise CoSnarksHipError("honk_co: scaling_stride must be 1 .. 2^28")
        edges = (edge_end - edge_begin) // 2
        m = edges if m is None else int(m)
        if (edge_idx is None and m != edges) or not 0 <= m <= edges:
            raise CoSnarksHipError("honk_co: m must be the number of edges of the range, or with an edge list at most that")
        self.curve, self.protocol, self.party, self.cols, self.edge_begin, self.edge_end = curve, protocol, party, list(cols), edge_begin, edge_end
        self.edge_idx, self.m, self.scaling, self.scaling_stride = edge_idx, m, scaling, scaling_stride
        self.params = _u64(params) if params is not None else None
        if self.params is not None and self.params.size != 4 * self.PARAMS[0]:
            raise CoSnarksHipError("honk_co: params are %s (%d elements of 4 words)" % (self.PARAMS[1], self.PARAMS[0]))
        self.ncomp = protocol + 1

    def common(self):
        return (self.curve, C.c_uint32(self.protocol), C.c_uint32(self.party), _devptr_array(self.cols), C.c_size_t(self.edge_begin),
                C.c_size_t(self.edge_end), _devptr(self.edge_idx), C.c_size_t(self.m))

    def scaled(self):
        return (_devptr(self.scaling), C.c_size_t(self.scaling_stride))

    def shares(self, count):
        """a DeviceBuffer of `count` batch vectors (7 m shares each)"""
        return DeviceBuffer(max(32, 32 * count * HONK_CO_POINTS * self.m * self.ncomp))

    def acc(self, elems, ncomp=None):
        return DeviceBuffer(32 * elems * (ncomp or self.ncomp))


def honk_co_select_edges(curve: int, selector, edge_begin: int, edge_end: int, edge_idx=None, count=None, stream=None):
    """csh_honk_co_select_edges_dev: selector = the q_arith or q_delta_range column. -> (edge_idx: uint32 per edge of the range, the kept
    e >> 1 in front; count: one uint32 word), made here unless given. The caller copies the count back."""
    if edge_begin < 0 or edge_begin % 2 or edge_end % 2 or not edge_begin < edge_end <= HONK_MAX_EDGE_END:
        raise CoSnarksHipError("honk_co_select_edges: edge_begin and edge_end must be even, edge_begin < edge_end <= 2^28")
    if edge_idx is None:
        edge_idx = DeviceBuffer(4 * ((edge_end - edge_begin) // 2))
    if count is None:
        count = DeviceBuffer(4)
    _check(lib().csh_honk_co_select_edges_dev(curve, _devptr(selector), C.c_size_t(edge_begin), C.c_size_t(edge_end), _devptr(edge_idx),
                                              _devptr(count), _stream(stream)))
    return edge_idx, count


def honk_co_arith(b: HonkCoBatch, mask=None, r0=None, r1=None, stream=None):
    """csh_honk_co_arith_dev: mask = 7 m elements for Rep3, None for protocol 0. -> (r0: 6 elements, a half share; r1: 5 shares)"""
    if (b.protocol == 1) != (mask is not None) and b.m:
        raise CoSnarksHipError("honk_co_arith: the mask vector is required for Rep3 and must be None for protocol 0")
    r0 = r0 if r0 is not None else b.acc(6, 1)
    r1 = r1 if r1 is not None else b.acc(5)
    _check(lib().csh_honk_co_arith_dev(*b.common(), *b.scaled(), _devptr(mask), _devptr(r0), _devptr(r1), _stream(stream)))
    return r0, r1


def honk_co_perm_operands(b: HonkCoBatch, lhs=None, rhs=None, stream=None):
    """csh_honk_co_perm_operands_dev -> (lhs, rhs), 4 * 7 m shares each"""
    lhs = lhs if lhs is not None else b.shares(4)
    rhs = rhs if rhs is not None else b.shares(4)
    _check(lib().csh_honk_co_perm_operands_dev(*b.common(), _p(b.params), _devptr(lhs), _devptr(rhs), _stream(stream)))
    return lhs, rhs


def honk_co_perm_operands2(b: HonkCoBatch, rhs=None, stream=None):
    """csh_honk_co_perm_operands2_dev -> rhs, 2 * 7 m shares"""
    rhs = rhs if rhs is not None else b.shares(2)
    _check(lib().csh_honk_co_perm_operands2_dev(*b.common(), _p(b.params), _devptr(rhs), _stream(stream)))
    return rhs


def honk_co_perm_finish(b: HonkCoBatch, prod, acc=None, stream=None):
    """csh_honk_co_perm_finish_dev: prod = 2 * 7 m shares -> acc = perm.r0 (6 shares), perm.r1 (3 shares)"""
    acc = acc if acc is not None else b.acc(9)
    _check(lib().csh_honk_co_perm_finish_dev(*b.common(), *b.scaled(), _devptr(prod), _devptr(acc), _stream(stream)))
    return acc


def honk_co_delta_operands(b: HonkCoBatch, lhs=None, stream=None):
    """csh_honk_co_delta_operands_dev -> lhs, 8 * 7 m shares"""
    lhs = lhs if lhs is not None else b.shares(8)
    _check(lib().csh_honk_co_delta_operands_dev(*b.common(), _devptr(lhs), _stream(stream)))
    return lhs


def honk_co_delta_sub_one(curve: int, protocol: int, party: int, sqr, m: int, stream=None):
    """csh_honk_co_delta_sub_one_dev: (+) -1 on the 8 * 7 m shares of sqr, in place"""
    if protocol not in (0, 1) or party not in (0, 1, 2) or not 0 <= m <= HONK_MAX_EDGE_END // 2:
        raise CoSnarksHipError("honk_co_delta_sub_one: protocol 0 or 1, party 0, 1 or 2, m at most 2^27")
    _check(lib().csh_honk_co_delta_sub_one_dev(curve, C.c_uint32(protocol), C.c_uint32(party), _devptr(sqr), C.c_size_t(m), _stream(stream)))
    return sqr


def honk_co_delta_finish(b: HonkCoBatch, mul, acc=None, stream=None):
    """csh_honk_co_delta_finish_dev: mul = 4 * 7 m shares -> acc = delta.r0 .. r3 (6 shares each)"""
    acc = acc if acc is not None else b.acc(24)
    _check(lib().csh_honk_co_delta_finish_dev(*b.common(), *b.scaled(), _devptr(mul), _devptr(acc), _stream(stream)))
    return acc


def honk_co_lookup_operands(b: HonkCoBatch, read_term=None, inverses=None, stream=None):
    """csh_honk_co_lookup_operands_dev -> (read_term, inverses), 7 m shares each"""
    read_term = read_term if read_term is not None else b.shares(1)
    inverses = inverses if inverses is not None else b.shares(1)
    _check(lib().csh_honk_co_lookup_operands_dev(*b.common(), _p(b.params), _devptr(read_term), _devptr(inverses), _stream(stream)))
    return read_term, inverses


def honk_co_lookup_mid(b: HonkCoBatch, write_inverse, r0=None, lhs=None, rhs=None, stream=None):
    """csh_honk_co_lookup_mid_dev: write_inverse = 7 m shares -> (r0: 5 shares; lhs, rhs: 2 * 7 m shares each)"""
    r0 = r0 if r0 is not None else b.acc(5)
    lhs = lhs if lhs is not None else b.shares(2)
    rhs = rhs if rhs is not None else b.shares(2)
    _check(lib().csh_honk_co_lookup_mid_dev(*b.common(), *b.scaled(), _p(b.params), _devptr(write_inverse), _devptr(r0), _devptr(lhs),
                                            _devptr(rhs), _stream(stream)))
    return r0, lhs, rhs


def honk_co_lookup_finish(b: HonkCoBatch, mul, acc=None, stream=None):
    """csh_honk_co_lookup_finish_dev: mul = 2 * 7 m shares -> acc = lookup.r1 (5 shares, no scaling), lookup.r2 (3 shares)"""
    acc = acc if acc is not None else b.acc(8)
    _check(lib().csh_honk_co_lookup_finish_dev(*b.common(), *b.scaled(), _p(b.params), _devptr(mul), _devptr(acc), _stream(stream)))
    return acc


# ---- the five gate relations on shares (csrc/honk_co_gates.hip): one wrapper per entry of include/cosnarks_hip.h ----------------------
class HonkCoGatesBatch(HonkCoBatch):
    """HonkCoBatch over the 19 columns of honk_sumcheck_accumulate_gates (eight share columns, eleven public ones) and its eight host
    parameters eta_1, eta_2, eta_3, curve_b, mat_internal_diag_m_1[0..4); edge_idx = the list of honk_co_select_edges on the relation's
    own selector. The same checks, before any call."""
    COLUMNS = HONK_GATES_COLUMNS
    PARAMS = (HONK_GATES_PARAMS, "eta_1, eta_2, eta_3, curve_b, mat_internal_diag_m_1[0..4)")

    def need_params(self, what):
        if self.params is None:
            raise CoSnarksHipError("%s: the batch has no params" % what)
        return _p(self.params)


def honk_co_ell_operands(b: HonkCoGatesBatch, lhs=None, rhs=None, stream=None):
    """csh_honk_co_ell_operands_dev -> (lhs, rhs), 7 * 7 m shares each"""
    lhs = lhs if lhs is not None else b.shares(7)
    rhs = rhs if rhs is not None else b.shares(7)
    _check(lib().csh_honk_co_ell_operands_dev(*b.common(), _devptr(lhs), _devptr(rhs), _stream(stream)))
    return lhs, rhs


def honk_co_ell_operands2(b: HonkCoGatesBatch, mul1, lhs=None, rhs=None, stream=None):
    """csh_honk_co_ell_operands2_dev: mul1 = 7 * 7 m shares -> (lhs, rhs), 5 * 7 m shares each"""
    par = b.need_params("honk_co_ell_operands2")
    lhs = lhs if lhs is not None else b.shares(5)
    rhs = rhs if rhs is not None else b.shares(5)
    _check(lib().csh_honk_co_ell_operands2_dev(*b.common(), par, _devptr(mul1), _devptr(lhs), _devptr(rhs), _stream(stream)))
    return lhs, rhs


def honk_co_ell_finish(b: HonkCoGatesBatch, mul1, mul2, acc=None, stream=None):
    """csh_honk_co_ell_finish_dev: mul1 = 7 * 7 m shares, mul2 = 5 * 7 m shares -> acc = elliptic.r0, r1 (6 shares each)"""
    acc = acc if acc is not None else b.acc(12)
    _check(lib().csh_honk_co_ell_finish_dev(*b.common(), *b.scaled(), _devptr(mul1), _devptr(mul2), _devptr(acc), _stream(stream)))
    return acc


def honk_co_mem_operands(b: HonkCoGatesBatch, lhs=None, rhs=None, rhs2=None, stream=None):
    """csh_honk_co_mem_operands_dev -> (lhs, rhs: 6 * 7 m shares each; rhs2: 7 m shares)"""
    par = b.need_params("honk_co_mem_operands")
    lhs = lhs if lhs is not None else b.shares(6)
    rhs = rhs if rhs is not None else b.shares(6)
    rhs2 = rhs2 if rhs2 is not None else b.shares(1)
    _check(lib().csh_honk_co_mem_operands_dev(*b.common(), par, _devptr(lhs), _devptr(rhs), _devptr(rhs2), _stream(stream)))
    return lhs, rhs, rhs2


def honk_co_mem_finish(b: HonkCoGatesBatch, mul, mul2, acc=None, stream=None):
    """csh_honk_co_mem_finish_dev: mul = 6 * 7 m shares, mul2 = 7 m shares -> acc = memory.r0 .. r5 (6 shares each)"""
    par = b.need_params("honk_co_mem_finish")
    acc = acc if acc is not None else b.acc(36)
    _check(lib().csh_honk_co_mem_finish_dev(*b.common(), *b.scaled(), par, _devptr(mul), _devptr(mul2), _devptr(acc), _stream(stream)))
    return acc


def honk_co_nnf_operands(b: HonkCoGatesBatch, lhs=None, rhs=None, stream=None):
    """csh_honk_co_nnf_operands_dev -> (lhs, rhs), 5 * 7 m shares each"""
    lhs = lhs if lhs is not None else b.shares(5)
    rhs = rhs if rhs is not None else b.shares(5)
    _check(lib().csh_honk_co_nnf_operands_dev(*b.common(), _devptr(lhs), _devptr(rhs), _stream(stream)))
    return lhs, rhs


def honk_co_nnf_finish(b: HonkCoGatesBatch, mul, acc=None, stream=None):
    """csh_honk_co_nnf_finish_dev: mul = 5 * 7 m shares -> acc = nnf.r0 (6 shares)"""
    acc = acc if acc is not None else b.acc(6)
    _check(lib().csh_honk_co_nnf_finish_dev(*b.common(), *b.scaled(), _devptr(mul), _devptr(acc), _stream(stream)))
    return acc


def honk_co_pos_ext_operands(b: HonkCoGatesBatch, s=None, stream=None):
    """csh_honk_co_pos_ext_operands_dev -> s, 4 * 7 m shares"""
    s = s if s is not None else b.shares(4)
    _check(lib().csh_honk_co_pos_ext_operands_dev(*b.common(), _devptr(s), _stream(stream)))
    return s


def honk_co_pos_ext_finish(b: HonkCoGatesBatch, u, acc=None, stream=None):
    """csh_honk_co_pos_ext_finish_dev: u = s^5, 4 * 7 m shares -> acc = poseidon2_external.r0 .. r3 (7 shares each)"""
    acc = acc if acc is not None else b.acc(28)
    _check(lib().csh_honk_co_pos_ext_finish_dev(*b.common(), *b.scaled(), _devptr(u), _devptr(acc), _stream(stream)))
    return acc


def honk_co_pos_int_operands(b: HonkCoGatesBatch, s1=None, stream=None):
    """csh_honk_co_pos_int_operands_dev -> s1, 7 m shares"""
    s1 = s1 if s1 is not None else b.shares(1)
    _check(lib().csh_honk_co_pos_int_operands_dev(*b.common(), _devptr(s1), _stream(stream)))
    return s1


def honk_co_pos_int_finish(b: HonkCoGatesBatch, u1, acc=None, stream=None):
    """csh_honk_co_pos_int_finish_dev: u1 = s1^5, 7 m shares -> acc = poseidon2_internal.r0 .. r3 (7 shares each)"""
    par = b.need_params("honk_co_pos_int_finish")
    acc = acc if acc is not None else b.acc(28)
    _check(lib().csh_honk_co_pos_int_finish_dev(*b.common(), *b.scaled(), par, _devptr(u1), _devptr(acc), _stream(stream)))
    return acc


# ---- batched Poseidon2 (csrc/poseidon2.hip): one wrapper per entry of include/cosnarks_hip.h -----------------------------------------
POSEIDON2_SPONGE, POSEIDON2_COMPRESSION = 0, 1


def _poseidon2_tree_rules(what, t, arity, mode, n_leaves=1):
    if mode not in (POSEIDON2_SPONGE, POSEIDON2_COMPRESSION):
        raise CoSnarksHipError("%s: mode must be 0 (sponge) or 1 (compression)" % what)
    if arity < 2 or (t <= arity if mode == POSEIDON2_SPONGE else t < arity):
        raise CoSnarksHipError("%s: arity must be at least 2, below t in sponge mode and at most t in compression mode" % what)
    v = n_leaves
    while v > 1 and v % arity == 0:
        v //= arity
    if v != 1:
        raise CoSnarksHipError("%s: n_leaves must be a power of the arity" % what)


class Poseidon2Params:
    """csh_poseidon2_params_create: one parameter set on the device (the fields of the reference's Poseidon2Params; the library builds in
    none). rc_external: (rounds_f_beginning + rounds_f_end) * t host elements, rc_internal: rounds_p, diag_m_1: t."""

    def __init__(self, curve: int, t: int, rounds_f_beginning: int, rounds_f_end: int, rounds_p: int, rc_external, rc_internal, diag_m_1):
        if t not in (2, 3, 4):
            raise CoSnarksHipError("Poseidon2Params: t must be 2, 3 or 4 (d = 5)")
        if min(rounds_f_beginning, rounds_f_end, rounds_p) < 0:
            raise CoSnarksHipError("Poseidon2Params: a negative round count")
        ext, inn, diag = _u64(rc_external), _u64(rc_internal), _u64(diag_m_1)
        if ext.size != 4 * (rounds_f_beginning + rounds_f_end) * t or inn.size != 4 * rounds_p or diag.size != 4 * t:
            raise CoSnarksHipError("Poseidon2Params: rc_external holds (rounds_f_beginning + rounds_f_end) * t elements, rc_internal rounds_p, diag_m_1 t")
        self.curve, self.t, self.rf_b, self.rf_e, self.rp = curve, t, rounds_f_beginning, rounds_f_end, rounds_p
        self.h = C.c_void_p()
        _check(lib().csh_poseidon2_params_create(curve, C.c_uint32(t), C.c_uint32(rounds_f_beginning), C.c_uint32(rounds_f_end), C.c_uint32(rounds_p),
                                                 _p(ext) if ext.size else None, _p(inn) if inn.size else None, _p(diag), C.byref(self.h)))

    @property
    def rounds(self):
        return self.rf_b + self.rp + self.rf_e

    def round_entries(self, r: int, n_perm: int) -> int:
        """precomputation entries round r consumes: n_perm * t in an external round, n_perm in an internal one"""
        return n_perm * self.t if (r < self.rf_b or r >= self.rf_b + self.rp) else n_perm

    def free(self):
        if self.h:
            lib().csh_poseidon2_params_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def poseidon2_permute(params: Poseidon2Params, state, n_perm: int, out=None, stream=None):
    """csh_poseidon2_permute_dev: n_perm states of t elements; out (default: in place) is returned."""
    out = out if out is not None else state
    _check(lib().csh_poseidon2_permute_dev(params.h, _devptr(state), C.c_size_t(n_perm), _devptr(out), _stream(stream)))
    return out


def poseidon2_merkle(params: Poseidon2Params, arity: int, mode: int, leaves, n_leaves: int, root=None, work=None, stream=None):
    """csh_poseidon2_merkle_dev: the root (one element, returned as a DeviceBuffer) of n_leaves = arity^k leaves."""
    _poseidon2_tree_rules("poseidon2_merkle", params.t, arity, mode, n_leaves)
    root = root if root is not None else DeviceBuffer(32)
    if work is None and n_leaves > arity:
        work = DeviceBuffer(32 * 2 * (n_leaves // arity))
    _check(lib().csh_poseidon2_merkle_dev(params.h, C.c_uint32(arity), C.c_uint32(mode), _devptr(leaves), C.c_size_t(n_leaves), _devptr(root),
                                          _devptr(work), _stream(stream)))
    return root


def poseidon2_co_round(curve: int, protocol: int, party: int, params: Poseidon2Params, step: int, state, n_perm: int, y, precomp,
                       precomp_offset: int, open_out=None, ff_out=None, stream=None):
    """csh_poseidon2_co_round_dev: step `step` of 0 .. params.rounds on n_perm states of shares, in place. y: the opened values of the round
    before (None at step 0); precomp: the five DeviceBuffers r, r^2, r^3, r^4, r^5; precomp_offset: the offset of round `step`.
    -> open_out (the shares to open; None at the last step)."""
    if protocol not in (0, 1) or party not in (0, 1, 2):
        raise CoSnarksHipError("poseidon2_co_round: protocol must be 0 (plain / Shamir) or 1 (Rep3), party_id 0, 1 or 2")
    if not 0 <= step <= params.rounds:
        raise CoSnarksHipError("poseidon2_co_round: step must be 0 .. rounds_f_beginning + rounds_p + rounds_f_end")
    if len(precomp) != 5:
        raise CoSnarksHipError("poseidon2_co_round: precomp holds the five vectors r, r^2, r^3, r^4, r^5")
    if step < params.rounds and open_out is None:
        open_out = DeviceBuffer(max(32 * (protocol + 1) * params.round_entries(step, n_perm), 32))
    _check(lib().csh_poseidon2_co_round_dev(curve, C.c_uint32(protocol), C.c_uint32(party), params.h, C.c_uint32(step), _devptr(state),
                                            C.c_size_t(n_perm), _devptr(y), _devptr_array(precomp), C.c_size_t(precomp_offset), _devptr(open_out),
                                            _devptr(ff_out), _stream(stream)))
    return open_out


def poseidon2_layer_next(curve: int, ncomp: int, t: int, arity: int, mode: int, state, ff, length: int, next_out=None, stream=None):
    """csh_poseidon2_layer_next_dev: the length / arity states of the next layer of a collaborative tree (length == 1: the root's share)."""
    if t not in (2, 3, 4):
        raise CoSnarksHipError("poseidon2_layer_next: t must be 2, 3 or 4")
    _poseidon2_tree_rules("poseidon2_layer_next", t, arity, mode)
    if length < 1 or (length != 1 and length % arity):
        raise CoSnarksHipError("poseidon2_layer_next: len must be 1 or a multiple of the arity")
    if next_out is None:
        next_out = DeviceBuffer(32 * ncomp * (1 if length == 1 else length // arity * t))
    _check(lib().csh_poseidon2_layer_next_dev(curve, C.c_uint32(ncomp), C.c_uint32(t), C.c_uint32(arity), C.c_uint32(mode), _devptr(state),
                                              _devptr(ff), _devptr(next_out), C.c_size_t(length), _stream(stream)))
    return next_out


# ---- F::rand streams and DN07 double sharings (csrc/field_rand.hip, csrc/shamir_rng.hip) -------------------------------------------
SHAMIR_MAX_PARTIES = 16
_FIELD_RAND_MAX_CAND = 1 << 62


def _seed32(seed, what):
    b = bytes(seed)
    if len(b) != 32:
        raise CoSnarksHipError("%s: a seed is 32 bytes" % what)
    return b


def field_rand(curve: int, seed, cand_begin: int, n: int, out=None, stream=None):
    """csh_field_rand_dev: the first n accepted F::rand candidates of ChaCha12Rng::from_seed(seed) at or after candidate cand_begin
    -> (out DeviceBuffer of n elements, cand_end). Synchronises the stream."""
    seed = _seed32(seed, "field_rand")
    if curve not in (BN254, BLS12_381, BLS12_377):
        raise CoSnarksHipError("field_rand: field_of must be BN254, BLS12-381 or BLS12-377")
    if n < 0 or n > 1 << 28 or not 0 <= cand_begin <= _FIELD_RAND_MAX_CAND:
        raise CoSnarksHipError("field_rand: n must be 0 .. 2^28 and cand_begin 0 .. 2^62")
    if out is None:
        out = DeviceBuffer(max(32 * n, 32))
    elif isinstance(out, DeviceBuffer) and out.nbytes < 32 * n:
        raise CoSnarksHipError("field_rand: out holds fewer than n elements")
    end = C.c_uint64(0)
    _check(lib().csh_field_rand_dev(curve, seed, C.c_uint64(cand_begin), C.c_size_t(n), _devptr(out), C.byref(end), _stream(stream)))
    return out, end.value


def field_rand_plan(curve: int, n: int, cand_begin: int = 0):
    """csh_field_rand_plan -> (candidates of the first window, workgroups, candidates per workgroup, acceptance rate)"""
    out = (C.c_uint64 * 4)()
    _check(lib().csh_field_rand_plan(curve, C.c_size_t(n), C.c_uint64(cand_begin), out))
    return out[0], out[1], out[2], out[3] / 1e9


class ShamirRng:
    """csh_shamir_rng_t: one Shamir party's shared streams (seeds: num_parties - 1 seeds of 32 bytes, stream q shared with party q for
    q < id and q + 1 otherwise; positions in candidates), public matrices and the device buffers r_t / r_2t."""

    def __init__(self, curve: int, party_id: int, num_parties: int, threshold: int, seeds, positions=None):
        if curve not in (BN254, BLS12_381, BLS12_377):
            raise CoSnarksHipError("ShamirRng: field_of must be BN254, BLS12-381 or BLS12-377")
        if num_parties > SHAMIR_MAX_PARTIES:
            raise CoSnarksHipError("ShamirRng: num_parties exceeds 16, the limit of this library")
        if threshold < 1 or 2 * threshold + 1 > num_parties:
            raise CoSnarksHipError("ShamirRng: threshold must be at least 1 and 2 * threshold + 1 <= num_parties")
        if not 0 <= party_id < num_parties:
            raise CoSnarksHipError("ShamirRng: id must be below num_parties")
        seeds = [_seed32(s, "ShamirRng") for s in seeds]
        if len(seeds) != num_parties - 1 or (positions is not None and len(positions) != num_parties - 1):
            raise CoSnarksHipError("ShamirRng: num_parties - 1 seeds (and positions)")
        if positions is not None and any(not 0 <= int(x) <= _FIELD_RAND_MAX_CAND for x in positions):
            raise CoSnarksHipError("ShamirRng: a stream position exceeds 2^62")
        self.curve, self.id, self.n, self.t = curve, party_id, num_parties, threshold
        self.n_send = (num_parties - threshold - 2) + (num_parties - 2 * threshold - 1)  # wire vectors of one double share, t block then 2t block
        pos = (C.c_uint64 * (num_parties - 1))(*[int(x) for x in positions]) if positions is not None else None
        self.h = C.c_void_p()
        _check(lib().csh_shamir_rng_create(curve, C.c_uint32(party_id), C.c_uint32(num_parties), C.c_uint32(threshold), b"".join(seeds), pos, C.byref(self.h)))

    def positions(self):
        out = (C.c_uint64 * (self.n - 1))()
        _check(lib().csh_shamir_rng_positions(self.h, out))
        return list(out)

    def fork_seeds(self):
        """csh_shamir_rng_fork_seeds: one 32-byte seed draw from every shared stream (fork_with_pairs); positions advance by one"""
        out = C.create_string_buffer(32 * (self.n - 1))
        _check(lib().csh_shamir_rng_fork_seeds(self.h, out))
        return [out.raw[32 * q:32 * q + 32] for q in range(self.n - 1)]

    def __len__(self):
        v = C.c_size_t(0)
        _check(lib().csh_shamir_pairs_len(self.h, C.byref(v)))
        return v.value

    def double_share_local(self, amount: int, send=None, stream=None):
        """csh_shamir_double_share_local_dev -> send (DeviceBuffer of n_send * amount elements in wire order; None when nothing is sent)"""
        if not 1 <= amount <= 1 << 24:
            raise CoSnarksHipError("ShamirRng.double_share_local: amount must be 1 .. 2^24")
        if send is None and self.n_send:
            send = DeviceBuffer(32 * self.n_send * amount)
        _check(lib().csh_shamir_double_share_local_dev(self.h, C.c_size_t(amount), _devptr(send), _stream(stream)))
        return send

    def double_share_finish(self, amount: int, recv=None, stream=None):
        """csh_shamir_double_share_finish_dev: recv = n_send * amount received elements; appends amount * (threshold + 1) pairs"""
        if recv is None and self.n_send:
            raise CoSnarksHipError("ShamirRng.double_share_finish: recv is None but this party receives")
        _check(lib().csh_shamir_double_share_finish_dev(self.h, C.c_size_t(amount), _devptr(recv), _stream(stream)))

    def take(self, count: int, from_front: bool = False, r_t=None, r_2t=None, stream=None):
        """csh_shamir_pairs_take_dev -> (r_t, r_2t) DeviceBuffers of count elements: pops from the back (element i = the i-th pop) or
        the drain from the front"""
        if count < 0:
            raise CoSnarksHipError("ShamirRng.take: a negative count")
        r_t = r_t if r_t is not None else DeviceBuffer(max(32 * count, 32))
        r_2t = r_2t if r_2t is not None else DeviceBuffer(max(32 * count, 32))
        _check(lib().csh_shamir_pairs_take_dev(self.h, C.c_size_t(count), C.c_int(1 if from_front else 0), _devptr(r_t), _devptr(r_2t), _stream(stream)))
        return r_t, r_2t

    def free(self):
        if self.h:
            lib().csh_shamir_rng_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def rep3_local_mul_vec(curve: int, lhs_ab, rhs_ab, mask=None):
    l, r = _u64(lhs_ab), _u64(rhs_ab)
    n = l.size // 8
    m = _u64(mask) if mask is not None else None
    out = np.empty(n * 4, dtype=np.uint64)
    _check(lib().csh_rep3_local_mul_vec(curve, _p(l), _p(r), _p(m), _p(out), C.c_size_t(n)))
    return out


def rep3_to_shamir_vec(curve: int, in_ab, x, y):
    a = _u64(in_ab)
    n = a.size // 8
    out = np.empty(n * 4, dtype=np.uint64)
    xx, yy = _u64(x), _u64(y)
    _check(lib().csh_rep3_to_shamir_vec(curve, _p(a), _p(xx), _p(yy), _p(out), C.c_size_t(n)))
    return out


def lincomb(curve: int, shares, coeffs):
    sh = [_u64(s) for s in shares]
    k = len(sh)
    n = sh[0].size // 4
    arr = (C.c_void_p * k)(*[s.ctypes.data for s in sh])
    co = _u64(coeffs)
    out = np.empty(n * 4, dtype=np.uint64)
    _check(lib().csh_lincomb(curve, arr, _p(co), C.c_size_t(k), _p(out), C.c_size_t(n)))
    return out


def groth16_h(dom: Domain, shift, protocol: int, a, b, mask_c=None, mask_ab=None):
    a, b = _u64(a).copy(), _u64(b).copy()
    out = np.empty(dom.n * 4, dtype=np.uint64)
    sh = _u64(shift)
    mc = _u64(mask_c) if mask_c is not None else None
    mab = _u64(mask_ab) if mask_ab is not None else None
    _check(lib().csh_groth16_h(dom.h, _p(sh), int(protocol), _p(a), _p(b), _p(mc), _p(mab), _p(out)))
    return out


def groth16_witness_map_masks(dom: Domain, shift, protocol: int, party: int, a: "Matrix", b: "Matrix", num_constraints: int, public, witness,
                              mask_c=None, mask_ab=None, fresh_output: bool = True):
    """csh_groth16_witness_map_masks: CircomReduction::witness_map_from_matrices in one call, Rep3 masks handed over by the caller.
    fresh_output: h is written into memory that was allocated but never touched (np.empty), as the Rust shim does."""
    pub, wit, sh = _u64(public), _u64(witness), _u64(shift)
    comp = 2 if protocol == 1 else 1
    out = np.empty(dom.n * 4, dtype=np.uint64) if fresh_output else np.zeros(dom.n * 4, dtype=np.uint64)
    mc = _u64(mask_c) if mask_c is not None else None
    mab = _u64(mask_ab) if mask_ab is not None else None
    _check(lib().csh_groth16_witness_map_masks(dom.h, _p(sh), int(protocol), int(party), a.h, b.h, C.c_size_t(num_constraints), _p(pub),
                                               C.c_size_t(pub.size // 4), _p(wit), C.c_size_t(wit.size // (4 * comp)), _p(mc), _p(mab), _p(out)))
    return out


def groth16_witness_map_seeded(dom: Domain, shift, protocol: int, party: int, a: "Matrix", b: "Matrix", num_constraints: int, public, witness,
                               seed1=None, off1: int = 0, seed2=None, off2: int = 0):
    """csh_groth16_witness_map: the same map with the masks generated on the device from the party's two ChaCha12 keys."""
    pub, wit, sh = _u64(public), _u64(witness), _u64(shift)
    comp = 2 if protocol == 1 else 1
    out = np.empty(dom.n * 4, dtype=np.uint64)
    s1 = (C.c_uint8 * 32)(*seed1) if seed1 is not None else None
    s2 = (C.c_uint8 * 32)(*seed2) if seed2 is not None else None
    _check(lib().csh_groth16_witness_map(dom.h, _p(sh), int(protocol), int(party), a.h, b.h, C.c_size_t(num_constraints), _p(pub),
                                         C.c_size_t(pub.size // 4), _p(wit), C.c_size_t(wit.size // (4 * comp)), s1, C.c_uint64(off1), s2,
                                         C.c_uint64(off2), _p(out)))
    return out


def sync(stream=None):
    _check(lib().csh_sync(_stream(stream)))


class Event:
    def __init__(self):
        self.h = C.c_void_p()
        _check(lib().csh_event_create(C.byref(self.h)))

    def record(self, stream=None):
        _check(lib().csh_event_record(self.h, _stream(stream)))

    def elapsed_ms(self, stop: "Event") -> float:
        ms = C.c_float(0)
        _check(lib().csh_event_elapsed_ms(self.h, stop.h, C.byref(ms)))
        return ms.value

    def __del__(self):
        try:
            if self.h:
                lib().csh_event_destroy(self.h)
        except Exception:
            pass


class Matrix:
    """Device-resident CSR constraint-matrix side (csh_matrix_upload)."""

    def __init__(self, curve: int, rows):
        """rows: list of rows, each a list of (coeff_limbs (4 u64, Montgomery), column index)."""
        self.curve = curve
        row_ptr = np.zeros(len(rows) + 1, dtype=np.uint64)
        cols, vals = [], []
        for i, r in enumerate(rows):
            for c, idx in r:
                cols.append(idx)
                vals.append(np.asarray(c, dtype=np.uint64))
            row_ptr[i + 1] = len(cols)
        col = np.asarray(cols, dtype=np.uint32)
        val = np.concatenate(vals).astype(np.uint64) if vals else np.zeros(0, dtype=np.uint64)
        self.n_rows = len(rows)
        self.h = C.c_void_p()
        _check(lib().csh_matrix_upload(curve, _p(row_ptr), _p(col), _p(val), C.c_size_t(len(rows)), C.c_size_t(len(cols)), C.byref(self.h)))

    def evaluate(self, protocol: int, party: int, public, witness, n_out: int):
        pub, wit = _u64(public), _u64(witness)
        comp = 2 if protocol == 1 else 1
        n_wit = wit.size // (4 * comp)
        dp, dw = DeviceBuffer.from_host(pub), DeviceBuffer.from_host(wit if wit.size else np.zeros(4, dtype=np.uint64))
        out = DeviceBuffer(n_out * comp * 32)
        _check(lib().csh_evaluate_constraints_dev(self.h, protocol, party, dp.ptr, C.c_size_t(pub.size // 4), dw.ptr, C.c_size_t(n_wit), out.ptr, C.c_size_t(n_out), None))
        sync()
        return out.to_host()

    def free(self):
        if self.h:
            lib().csh_matrix_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
