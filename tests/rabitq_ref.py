"""Plain-numpy reference of the IVFRABITQ index (helper, not a test):
faiss's 1-bit RaBitQuantizer with the float-query estimator, fp64
arithmetic on fp32 inputs.

An entry is D/8 + 8 bytes: the sign bits of r = fl32(x - c) (bit j of the
vector is bit j & 7 of byte j >> 3), then the factors A and Mul as
little-endian fp32. c is the centroid of the entry's list.

Order: L2 ascending, inner product descending, ties by id ascending —
the engine's (score, id) key order.
"""
import numpy as np

EPS = float(np.finfo(np.float32).eps)          # FLT_EPSILON
U = 2.0 ** -23                                  # one fp32 ulp at 1.0


def code_size(D):
    return D // 8 + 8


# ------------------------------------------------------------------ encode
def residual_bits(x, c):
    """r = x - c in ONE fp32 subtraction; bits = r > 0 -> (r fp32, bool)."""
    x = np.asarray(x, dtype=np.float32)
    c = np.broadcast_to(np.asarray(c, dtype=np.float32), x.shape)
    r = (x - c).astype(np.float32)
    return r, r > 0


def factors(x, c, ip):
    """(A, Mul, sval) in float64 for rows x (n, D) against centroids c
    ((D,) or (n, D))."""
    x = np.asarray(x, dtype=np.float32)
    D = x.shape[1]
    c = np.broadcast_to(np.asarray(c, dtype=np.float32), x.shape)
    r32, bits = residual_bits(x, c)
    r = r32.astype(np.float64)
    n2 = (r * r).sum(axis=1)
    l1 = np.abs(r).sum(axis=1)
    xx = (x.astype(np.float64) ** 2).sum(axis=1)
    inv_norm = np.where(n2 < EPS, 1.0, 1.0 / np.sqrt(np.where(n2 < EPS, 1.0,
                                                              n2)))
    ndp = l1 * inv_norm / np.sqrt(D)
    inv_dp = np.where(np.abs(ndp) < EPS, 1.0,
                      1.0 / np.where(np.abs(ndp) < EPS, 1.0, ndp))
    A = n2 - xx if ip else n2
    Mul = inv_dp * np.sqrt(n2)
    sval = (bits * c.astype(np.float64)).sum(axis=1)
    return A, Mul, sval


def pack(bits, A, Mul):
    """bool (n, D), factors -> uint8 (n, D/8 + 8) entries."""
    bits = np.asarray(bits, dtype=bool)
    n, D = bits.shape
    out = np.empty((n, code_size(D)), dtype=np.uint8)
    out[:, :D // 8] = np.packbits(bits, axis=1, bitorder="little")
    f = np.stack([np.asarray(A, np.float64), np.asarray(Mul, np.float64)],
                 axis=1).astype("<f4")
    out[:, D // 8:] = f.view(np.uint8).reshape(n, 8)
    return out


def unpack(codes, D):
    """uint8 (n, D/8 + 8) -> (bits bool (n, D), A fp32 (n,), Mul fp32)."""
    codes = np.ascontiguousarray(codes, dtype=np.uint8).reshape(
        -1, code_size(D))
    bits = np.unpackbits(codes[:, :D // 8], axis=1,
                         bitorder="little").astype(bool)
    f = np.ascontiguousarray(codes[:, D // 8:]).view("<f4").reshape(-1, 2)
    return bits, f[:, 0].copy(), f[:, 1].copy()


def encode(x, c, ip):
    """-> (codes uint8 (n, D/8 + 8), sval float64 (n,))."""
    _, bits = residual_bits(x, c)
    A, Mul, sval = factors(x, c, ip)
    return pack(bits, A, Mul), sval


# ---------------------------------------------------------------- estimate
def estimate(q, c, bits, A, Mul, ip):
    """Direct form: scores float64 (n,) of one query q (D,) against n
    entries of the list with centroid c (D,)."""
    q = np.asarray(q, np.float64)
    c = np.asarray(c, np.float64)
    D = q.shape[0]
    qr = q - c
    dot = (np.asarray(bits, bool) * qr).sum(axis=1)
    fd = (2.0 * dot - qr.sum()) / np.sqrt(D)
    pre = np.asarray(A, np.float64) + (qr * qr).sum() \
        - 2.0 * np.asarray(Mul, np.float64) * fd
    return -0.5 * (pre - (q * q).sum()) if ip else pre


def estimate_decomposed(q, c, bits, A, Mul, sval, ip):
    """The form the scan kernel computes: a query-only sum over the set
    bits minus the entry's sval, and per-(query, list) scalars."""
    q = np.asarray(q, np.float64)
    c = np.asarray(c, np.float64)
    D = q.shape[0]
    dot = (np.asarray(bits, bool) * q).sum(axis=1) - np.asarray(sval,
                                                                np.float64)
    fd = (2.0 * dot - (q.sum() - c.sum())) / np.sqrt(D)
    qc2 = (q * q).sum() - 2.0 * (q * c).sum() + (c * c).sum()
    pre = np.asarray(A, np.float64) + qc2 \
        - 2.0 * np.asarray(Mul, np.float64) * fd
    return -0.5 * (pre - (q * q).sum()) if ip else pre


def scale(q, c, A, Mul, ip):
    """The absolute mass of the sums a fp32 kernel may form for one score:
    |A| + 2(|q|^2 + |c|^2) + 4|Mul|/sqrt(D) (|q|_1 + |c|_1) + [IP]|q|^2."""
    q = np.asarray(q, np.float64)
    c = np.asarray(c, np.float64)
    D = q.shape[0]
    qq, cc = (q * q).sum(), (c * c).sum()
    s = np.abs(np.asarray(A, np.float64)) + 2.0 * (qq + cc) \
        + 4.0 * np.abs(np.asarray(Mul, np.float64)) / np.sqrt(D) \
        * (np.abs(q).sum() + np.abs(c).sum())
    return s + qq if ip else s


def tol(q, c, A, Mul, ip):
    """(D + 16) 2^-23 scale: a fixed-order fp32 sum of D terms errs by at
    most D 2^-24 of its absolute mass; derived, not measured."""
    return (len(q) + 16) * U * scale(q, c, A, Mul, ip)


# ------------------------------------------------------------------ search
def candidates(q, cent, lists_ids, lists_codes, probes_row, ip,
               del_bitmap=None, eps=None):
    """Every live entry of the probed lists of ONE query ->
    (ids int64, scores float64, tols float64). Entries whose id carries
    the bit-63 delete mark or is set in del_bitmap (bool by id) are
    skipped, and so are probes outside [0, nlist). eps: tolerance =
    eps * scale instead of tol()."""
    q = np.asarray(q, np.float32)
    D = q.shape[0]
    nlist = len(lists_ids)
    ci, cs, ct = [], [], []
    for ln in np.asarray(probes_row).tolist():
        if ln < 0 or ln >= nlist or len(lists_ids[ln]) == 0:
            continue
        li = np.asarray(lists_ids[ln], dtype=np.int64)
        live = li >= 0
        if del_bitmap is not None:
            live &= ~np.asarray(del_bitmap, dtype=bool)[np.where(li >= 0,
                                                                 li, 0)]
        if not live.any():
            continue
        bits, A, Mul = unpack(np.asarray(lists_codes[ln])[live], D)
        ci.append(li[live])
        cs.append(estimate(q, cent[ln], bits, A, Mul, ip))
        sc = scale(q, cent[ln], A, Mul, ip)
        ct.append(sc * eps if eps is not None else sc * (D + 16) * U)
    if not ci:
        z = np.empty(0)
        return np.empty(0, dtype=np.int64), z, z
    return np.concatenate(ci), np.concatenate(cs), np.concatenate(ct)


def topk(ids, scores, k, ip):
    """top-k by (score, id): -> (float32 scores, int64 ids) padded with
    -1.0 / -1 as the engine pads."""
    od = np.full(k, -1.0, dtype=np.float32)
    oi = np.full(k, -1, dtype=np.int64)
    order = np.lexsort((ids, -scores if ip else scores))[:k]
    od[:order.size] = scores[order]
    oi[:order.size] = ids[order]
    return od, oi


def search(q, cent, lists_ids, lists_codes, probes, k, ip, del_bitmap=None):
    """-> (float32 scores, int64 ids), both (nq, k)."""
    nq = len(q)
    od = np.empty((nq, k), dtype=np.float32)
    oi = np.empty((nq, k), dtype=np.int64)
    for r in range(nq):
        ids, sc, _ = candidates(q[r], cent, lists_ids, lists_codes,
                                probes[r], ip, del_bitmap)
        od[r], oi[r] = topk(ids, sc, k, ip)
    return od, oi


def brute(q, base, k, ip, del_bitmap=None):
    """Exact float64 top-k over the rows of base (ids = row numbers):
    squared L2 ascending or inner product descending, ties by id."""
    q = np.asarray(q, np.float64)
    base = np.asarray(base, np.float64)
    ids = np.arange(base.shape[0], dtype=np.int64)
    if del_bitmap is not None:
        ids = ids[~np.asarray(del_bitmap, dtype=bool)[:base.shape[0]]]
    od = np.empty((len(q), k), dtype=np.float32)
    oi = np.empty((len(q), k), dtype=np.int64)
    for r in range(len(q)):
        b = base[ids]
        sc = b @ q[r] if ip else ((b - q[r]) ** 2).sum(axis=1)
        od[r], oi[r] = topk(ids, sc, k, ip)
    return od, oi


def check_row(got_d, got_i, cand_ids, cand_scores, cand_tol, ip):
    """Tolerance-aware comparison of one output row against the reference
    candidates of that query. Asserts:
    (a) the row is sorted by (score, id) and padding is at the end;
    (b) every returned id is a candidate and its score is within that
        candidate's tolerance of the reference score;
    (c) no unreturned candidate beats the last returned score by more
        than its tolerance;
    (d) the count of non-padding results is min(k, candidates)."""
    got_d = np.asarray(got_d, np.float64)
    got_i = np.asarray(got_i, np.int64)
    k = got_i.shape[0]
    n = int((got_i >= 0).sum())
    assert n == min(k, cand_ids.size), (n, k, cand_ids.size)          # (d)
    assert np.all(got_i[:n] >= 0) and np.all(got_i[n:] == -1)
    assert len(set(got_i[:n].tolist())) == n, "duplicate ids"
    sgn = -1.0 if ip else 1.0
    s = sgn * got_d[:n]
    for j in range(1, n):                                              # (a)
        assert s[j - 1] < s[j] or (s[j - 1] == s[j] and
                                   got_i[j - 1] < got_i[j]), (j, got_d[:n])
    pos = {int(i): p for p, i in enumerate(cand_ids.tolist())}
    for j in range(n):                                                 # (b)
        assert int(got_i[j]) in pos, f"id {got_i[j]} is not a candidate"
        p = pos[int(got_i[j])]
        assert abs(got_d[j] - cand_scores[p]) <= cand_tol[p], (
            got_i[j], got_d[j], cand_scores[p], cand_tol[p])
    if n and cand_ids.size > n:                                        # (c)
        rest = np.ones(cand_ids.size, dtype=bool)
        rest[[pos[int(i)] for i in got_i[:n]]] = False
        worst = s[n - 1]
        bad = sgn * cand_scores[rest] < worst - cand_tol[rest]
        assert not bad.any(), (
            cand_ids[rest][bad][:5], cand_scores[rest][bad][:5], got_d[n - 1])
