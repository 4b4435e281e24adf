"""Plain numpy references for the kernel-level parity tests
(tests/test_gpu_kernels.py). No GPU, no ctypes: everything here is
checked on the CPU by tests/test_kernel_refs.py.

The selection reference has no selection algorithm of its own: it
encodes the u64 (dist, id) keys of csrc/select.hpp, sorts them and cuts.

Exact comparison of approximate-order kernels rests on grid inputs
(`grid`): every value is i/8 with integer |i| <= 8, so products are
multiples of 2^-6 with |p| <= 1 and squared differences are multiples of
2^-6 with value <= 4. For d <= 768 every partial sum is an integer count
of 2^-6 units below 2^24 — exactly representable in fp32 — so EVERY
accumulation order (MFMA, shuffle trees, sequential fmaf) gives the same
bits as a float64 reference.

TEST INFRASTRUCTURE ONLY — never part of the product path."""
import numpy as np

from vearch_amd.merge import _f32_key

EMPTY = 2 ** 64 - 1
_EMPTY = np.uint64(EMPTY)
_M32 = np.uint64(0xFFFFFFFF)

FLT_MAX = float(np.finfo(np.float32).max)
SUBNORMAL = 2.0 ** -140
# the special-value row of the selection tests (contains one exact tie)
SPECIALS = np.array(
    [-np.inf, -FLT_MAX, -3.0, -SUBNORMAL, 0.0, SUBNORMAL, 1.0, 1.0,
     FLT_MAX, np.inf], dtype=np.float32)


# ------------------------------------------------------------------ keys
def key_encode(dist_f32, id_u32, ip):
    """u64 key of select.hpp: (monotone u32 image of dist, inverted for
    inner product) << 32 | id. Ascending key == best first."""
    dist = np.asarray(dist_f32, dtype=np.float32)
    dk = _f32_key(dist)
    if ip:
        dk = _M32 - dk
    ids = np.asarray(id_u32).astype(np.uint64) & _M32
    return (dk << np.uint64(32)) | ids


def key_decode(keys, ip):
    """(dist f32, id int64) of each key; EMPTY -> (-1.0, -1)."""
    keys = np.asarray(keys, dtype=np.uint64)
    empty = keys == _EMPTY
    dk = (keys >> np.uint64(32)).astype(np.uint32)
    if ip:
        dk = ~dk
    u = np.where((dk & np.uint32(0x80000000)) != 0,
                 dk & np.uint32(0x7FFFFFFF), ~dk).astype(np.uint32)
    dist = np.where(empty, np.float32(-1.0), u.view(np.float32))
    ids = np.where(empty, np.int64(-1),
                   (keys & _M32).astype(np.int64))
    return dist.astype(np.float32), ids


def topk_keys(dist, ids, k2, ip, deleted=None, seed_keys=None):
    """Reference top-k2 of one row: encode, drop deleted ids, append the
    seed keys, sort ascending, cut to k2, pad with EMPTY.
    deleted: optional bool array indexed by id (True = deleted)."""
    dist = np.asarray(dist, dtype=np.float32).ravel()
    ids = np.asarray(ids).ravel().astype(np.int64)
    keys = key_encode(dist, ids, ip)
    if deleted is not None:
        keys = keys[~np.asarray(deleted, dtype=bool)[ids]]
    if seed_keys is not None:
        keys = np.concatenate(
            [keys, np.asarray(seed_keys, dtype=np.uint64).ravel()])
    keys = np.sort(keys)[:k2]
    out = np.full(k2, _EMPTY, dtype=np.uint64)
    out[:keys.size] = keys
    return out


def topk_keys_rows(dist, ids, k2, ip, deleted=None, seed_keys=None):
    """topk_keys over the rows of a 2-D dist matrix (ids shared)."""
    dist = np.asarray(dist, dtype=np.float32)
    return np.stack([
        topk_keys(dist[r], ids, k2, ip, deleted,
                  None if seed_keys is None else seed_keys[r])
        for r in range(dist.shape[0])])


def bitmap_words(deleted):
    """u32-word delete bitmap (bit id&31 of word id>>5) of a bool array."""
    deleted = np.asarray(deleted, dtype=bool)
    nw = (deleted.size + 31) // 32
    bits = np.zeros(nw * 32, dtype=np.uint64)
    bits[:deleted.size] = deleted
    w = (bits.reshape(nw, 32) << np.arange(32, dtype=np.uint64)).sum(axis=1)
    return w.astype(np.uint32)


# ------------------------------------------------------------ grid inputs
def grid(shape, seed):
    """f32 values i/8, integer i in [-8, 8] (see the module docstring)."""
    rng = np.random.default_rng(seed)
    return (rng.integers(-8, 9, size=shape) / 8.0).astype(np.float32)


def _exact_f32(x64):
    x32 = x64.astype(np.float32)
    assert np.array_equal(x32.astype(np.float64), x64), (
        "float64 reference is not exactly representable in fp32: the "
        "inputs are not on the exact grid")
    return x32


def dots_f64(a, b):
    """float64 a @ b.T of f32 inputs."""
    return np.asarray(a, np.float64) @ np.asarray(b, np.float64).T


def dots_exact(a, b):
    """a @ b.T for grid inputs, asserted exact in fp32."""
    return _exact_f32(dots_f64(a, b))


def norms_exact(a):
    a = np.asarray(a, np.float64)
    return _exact_f32((a * a).sum(axis=1))


def l2_from_dots(dots, qn, bn):
    """fmaf(-2, dot, qn + bn) per element, in float64 rounded once to
    fp32. Only exact on grid inputs — asserted (the inner qn + bn, which
    the kernels round to fp32 on its own, included)."""
    dots = np.asarray(dots, np.float64)
    s = (np.asarray(qn, np.float64)[:, None] +
         np.asarray(bn, np.float64)[None, :])
    _exact_f32(s)
    return _exact_f32(s - 2.0 * dots)


def l2_exact(q, base):
    """sum((q - b)^2) for grid inputs, asserted exact in fp32."""
    q = np.asarray(q, np.float64)
    base = np.asarray(base, np.float64)
    d = q[:, None, :] - base[None, :, :]
    return _exact_f32((d * d).sum(axis=2))


# -------------------------------------------------------------- PQ encode
def pq_encode_ref(x, codebooks, M, ksub):
    """codes[i][m] = lowest j minimising ||x_im - cb[m][j]||^2, float64
    brute force (exact on grid inputs, so ties are real ties)."""
    x = np.asarray(x, np.float64)
    n, d = x.shape
    dsub = d // M
    cb = np.asarray(codebooks, np.float64).reshape(M, ksub, dsub)
    codes = np.empty((n, M), dtype=np.uint8)
    for m in range(M):
        diff = x[:, None, m * dsub:(m + 1) * dsub] - cb[m][None, :, :]
        dist = (diff * diff).sum(axis=2)
        _exact_f32(dist)
        codes[:, m] = np.argmin(dist, axis=1)  # first minimum = lowest j
    return codes


def pack4(codes):
    """8-bit-form 4-bit codes (n, M) -> packed (n, M/2): byte b holds code
    2b in bits 0-3 and code 2b+1 in bits 4-7."""
    codes = np.asarray(codes, dtype=np.uint8)
    return (codes[:, 0::2] | (codes[:, 1::2] << 4)).astype(np.uint8)


def unpack4(packed):
    """inverse of pack4: (n, M/2) bytes -> (n, M) codes below 16."""
    packed = np.asarray(packed, dtype=np.uint8)
    out = np.empty((packed.shape[0], 2 * packed.shape[1]), dtype=np.uint8)
    out[:, 0::2] = packed & 15
    out[:, 1::2] = packed >> 4
    return out


# ------------------------------------------------------------- ADC chains
def adc_chain(start, table, codes):
    """start[i] + table[0][codes[i][0]] + table[1][codes[i][1]] + ...: one
    fp32 add per sub-quantizer in ascending m, rounded after every add.
    start: f32 scalar or (n,); table (M, ksub) f32; codes (n, M)."""
    table = np.asarray(table, dtype=np.float32)
    codes = np.asarray(codes)
    acc = np.broadcast_to(np.asarray(start, dtype=np.float32),
                          codes.shape[:1]).copy()
    for m in range(table.shape[0]):
        acc = (acc + table[m, codes[:, m]]).astype(np.float32)
    return acc


def sterm_ref(btab, codes, asg):
    """gk::pq_sterm: out[i] = adc_chain(0, btab[asg[i]], codes[i]); 0.0
    where asg[i] is outside [0, nlist). btab (nlist, M, ksub), codes (n, M)
    one code per byte, asg (n,) ints."""
    btab = np.asarray(btab, dtype=np.float32)
    codes = np.asarray(codes)
    asg = np.asarray(asg)
    out = np.zeros(codes.shape[0], dtype=np.float32)
    for ln in range(btab.shape[0]):
        sel = asg == ln
        out[sel] = adc_chain(np.float32(0.0), btab[ln], codes[sel])
    return out
