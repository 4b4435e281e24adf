"""Plain-numpy reference of the BINARYIVF index (helper, not a test).

Vectors are uint8 arrays of d/8 bytes; bit i of a vector is
(byte[i >> 3] >> (i & 7)) & 1. The bit order does not matter for a Hamming
distance, only that both sides use the same one. Every order is the
engine's (dist, id) ascending rule; all results are exact integers.
"""
import numpy as np


def hamming(a, b):
    """(na, nb) int64 matrix of Hamming distances between the rows of the
    uint8 arrays a (na, nbytes) and b (nb, nbytes)."""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    b = np.ascontiguousarray(b, dtype=np.uint8)
    assert a.ndim == 2 and b.ndim == 2 and a.shape[1] == b.shape[1]
    out = np.empty((a.shape[0], b.shape[0]), dtype=np.int64)
    step = max(1, (1 << 22) // max(1, b.shape[0] * b.shape[1]))
    for i in range(0, a.shape[0], step):
        x = a[i:i + step, None, :] ^ b[None, :, :]
        out[i:i + step] = np.unpackbits(x, axis=2).sum(axis=2)
    return out


def assign(x, cent):
    """nearest centroid per row of x, ties to the lowest list number."""
    return hamming(x, cent).argmin(axis=1).astype(np.int64)


def coarse(q, cent, nprobe):
    """top-nprobe centroids per query by (dist, list) ascending ->
    (float32 dists, int64 lists), both (nq, nprobe)."""
    h = hamming(q, cent)
    lists = np.empty((h.shape[0], nprobe), dtype=np.int64)
    for r in range(h.shape[0]):
        lists[r] = np.lexsort((np.arange(h.shape[1]), h[r]))[:nprobe]
    return np.take_along_axis(h, lists, axis=1).astype(np.float32), lists


def search(q, lists_ids, lists_codes, probes, k, del_bitmap=None):
    """Scan the probed lists of every query: entries whose id carries the
    bit-63 delete mark, or whose id is set in del_bitmap (bool array
    indexed by id), are skipped; probes outside [0, nlist) are skipped.
    -> (float32 dists, int64 ids), (nq, k), top-k by (dist, id) ascending,
    padded with -1.0 / -1."""
    q = np.ascontiguousarray(q, dtype=np.uint8)
    nq = q.shape[0]
    nlist = len(lists_ids)
    od = np.full((nq, k), -1.0, dtype=np.float32)
    oi = np.full((nq, k), -1, dtype=np.int64)
    for r in range(nq):
        ids, codes = [], []
        for ln in np.asarray(probes[r]).tolist():
            if ln < 0 or ln >= nlist or len(lists_ids[ln]) == 0:
                continue
            li = np.asarray(lists_ids[ln], dtype=np.int64)
            live = li >= 0
            if del_bitmap is not None:
                live &= ~np.asarray(del_bitmap, dtype=bool)[
                    np.where(li >= 0, li, 0)]
            ids.append(li[live])
            codes.append(np.asarray(lists_codes[ln], dtype=np.uint8)[live])
        if not ids:
            continue
        ids = np.concatenate(ids)
        if ids.size == 0:
            continue
        h = hamming(q[r:r + 1], np.concatenate(codes))[0]
        order = np.lexsort((ids, h))[:k]
        od[r, :order.size] = h[order]
        oi[r, :order.size] = ids[order]
    return od, oi


def brute(q, base, k, del_bitmap=None):
    """exact top-k over all rows of base (ids = row numbers)."""
    ids = np.arange(base.shape[0], dtype=np.int64)
    return search(q, [ids], [base], np.zeros((len(q), 1), dtype=np.int64), k,
                  del_bitmap)
