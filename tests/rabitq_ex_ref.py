"""Plain-numpy reference of the multi-bit IVFRABITQ code (helper, not a
test): nb_bits B = 4 or 8, L = 2^(B-1). Candidate codes in float32, one
rounded operation at a time (bit for bit); everything else fp64 on the
fp32 inputs. An entry is D*B/8 + 8 bytes: the codes u_j (B = 4: low nibble
first within a byte; B = 8: byte j), then A and Mul as little-endian fp32.
"""
import numpy as np

from rabitq_ref import EPS, U, brute, check_row, topk  # noqa: F401


def code_size(D, B):
    return D * B // 8 + 8


def cb(B):
    return (2 ** B - 1) / 2.0


def candidates32(r32, B):
    """r32 float32 (n, D) -> magnitudes m int64 (32, n, D): candidate i has
    the scale s_i = fl32(g_i / rmax), g_i = L (i + 1) / 8."""
    L = 1 << (B - 1)
    a = np.abs(np.asarray(r32, np.float32))
    rmax = a.max(axis=1, keepdims=True)
    out = np.zeros((32,) + a.shape, dtype=np.int64)
    nz = rmax[:, 0] > 0
    for i in range(32):
        s = (np.float32(L * (i + 1) / 8.0) / rmax[nz]).astype(np.float32)
        out[i, nz] = np.minimum(
            L - 1, np.floor((a[nz] * s).astype(np.float32)).astype(np.int64))
    return out


def objective(m, r32):
    """fp64 num^2 / den of magnitudes m (..., n, D)."""
    num = ((m + 0.5) * np.abs(np.asarray(r32, np.float64))).sum(axis=-1)
    return num * num / ((2 * m + 1) ** 2).sum(axis=-1)


def codes_of(m, r32, B):
    L = 1 << (B - 1)
    return np.where(np.asarray(r32) > 0, L + m, L - 1 - m).astype(np.int64)


def factors(u, x, c, B, ip):
    """fp64 (A, Mul, sval) of codes u (n, D) for rows x against c."""
    x = np.asarray(x, np.float32)
    c = np.broadcast_to(np.asarray(c, np.float32), x.shape)
    r = (x - c).astype(np.float32).astype(np.float64)
    n2 = (r * r).sum(axis=1)
    wr = ((u - cb(B)) * r).sum(axis=1)
    Mul = np.where(np.abs(wr) < EPS, 1.0, n2 / np.where(wr == 0, 1.0, wr))
    A = n2 - (x.astype(np.float64) ** 2).sum(axis=1) if ip else n2
    return A, Mul, (u * c.astype(np.float64)).sum(axis=1)


def unpack(codes, D, B):
    """uint8 (n, D*B/8 + 8) -> (u int64 (n, D), A fp32 (n,), Mul fp32)."""
    codes = np.ascontiguousarray(codes, dtype=np.uint8).reshape(
        -1, code_size(D, B))
    body = codes[:, :D * B // 8].astype(np.int64)
    u = body if B == 8 else np.stack([body & 15, body >> 4],
                                     axis=2).reshape(-1, D)
    f = np.ascontiguousarray(codes[:, D * B // 8:]).view("<f4").reshape(-1, 2)
    return u, f[:, 0].copy(), f[:, 1].copy()


def estimate(q, c, u, A, Mul, B, ip):
    """scores float64 (n,) of query q (D,) against n entries of the list
    with centroid c (D,)."""
    q = np.asarray(q, np.float64)
    qr = q - np.asarray(c, np.float64)
    pre = np.asarray(A, np.float64) + (qr * qr).sum() - 2.0 * np.asarray(
        Mul, np.float64) * ((u * qr).sum(axis=1) - cb(B) * qr.sum())
    return -0.5 * (pre - (q * q).sum()) if ip else pre


def scale(q, c, A, Mul, B, ip):
    """|A| + 2(|q|^2 + |c|^2) + 2|Mul| (2^B - 1 + cB)(|q|_1 + |c|_1)
    + [IP]|q|^2: the absolute mass of the sums behind one score."""
    q = np.asarray(q, np.float64)
    c = np.asarray(c, np.float64)
    qq = (q * q).sum()
    s = np.abs(np.asarray(A, np.float64)) + 2.0 * (qq + (c * c).sum()) \
        + 2.0 * np.abs(np.asarray(Mul, np.float64)) * (2 ** B - 1 + cb(B)) \
        * (np.abs(q).sum() + np.abs(c).sum())
    return s + qq if ip else s


def tol(q, c, A, Mul, B, ip):
    """(D + 16) 2^-23 scale, on the pattern of rabitq_ref.tol."""
    return (len(q) + 16) * U * scale(q, c, A, Mul, B, ip)


def candidates(q, cent, lists_ids, lists_codes, probes_row, B, ip, gone=None):
    """Every live entry of the probed lists of one query -> (ids, scores,
    tols); ids with the bit-63 mark or set in `gone` are skipped."""
    ci, cs, ct = [np.empty(0, np.int64)], [np.empty(0)], [np.empty(0)]
    for ln in np.asarray(probes_row).tolist():
        li = np.asarray(lists_ids[ln], dtype=np.int64)
        live = li >= 0
        if gone is not None:
            live &= ~np.asarray(gone, bool)[np.where(live, li, 0)]
        u, A, Mul = unpack(np.asarray(lists_codes[ln])[live], len(q), B)
        ci.append(li[live])
        cs.append(estimate(q, cent[ln], u, A, Mul, B, ip))
        ct.append(tol(q, cent[ln], A, Mul, B, ip))
    return np.concatenate(ci), np.concatenate(cs), np.concatenate(ct)
