"""k_ivfflat_scan on its own, through the kernel test hook: the
half-wave-per-vector layout (8 vectors per workgroup pass), the rotating
push lane and the flush check every 16th pass, against
kernel_refs.l2_exact / dots_exact + topk_keys.

Inputs sit on the exact grid of oracle.kernel_refs, so the kernel's
per-lane fmaf chains and shuffle tree give the bits of the float64
reference; keys are compared with np.array_equal.

Shapes: d = 4 (one float4 per vector: lane 0 of each half-wave works
alone), 36 (9 float4), 128 (exactly one round of the 32 lanes), 200 (50
float4: a second, partial round). 12 lists with sizes around the 8 vectors
of a pass and the 128 of a flush period, and one of 1100. Some vectors are
copied into other lists under other ids, so equal distances meet and the
order falls to the ids."""
import numpy as np
import pytest

from oracle import kernel_refs as kr

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 7, 8, 9, 127, 128, 129, 1100, 0, 9, 128]
NLIST = len(SIZES)
L = {s: SIZES.index(s) for s in set(SIZES)}  # first list of each size
E = [i for i, s in enumerate(SIZES) if s == 0]
NDOC = 4096
DIMS = [4, 36, 128, 200]

TABLES = {
    "rows5": np.array([
        [L[1100], L[129], L[128], L[127], L[9], L[8]],  # ~1400 live
        [-1, NLIST, E[0], E[1], -1, NLIST + 3],         # nothing to scan
        [L[7], L[7], -1, L[1], E[0], L[8]],             # a list twice
        [L[9], 10, L[1], NLIST, 11, L[1100]],           # the copies' lists
        [E[0], L[1], -1, -1, -1, -1],                   # one candidate
    ], dtype=np.int64),
    "nprobe1": np.array([[L[1100]], [E[0]], [-1], [L[1]], [NLIST]],
                        dtype=np.int64),
}


class Case:
    def __init__(self, d):
        self.d = d
        rng = np.random.default_rng(40 + d)
        self.queries = kr.grid((5, d), seed=d + 1)
        ids_pool = rng.permutation(NDOC)
        self.lists = []
        at = 0
        for li, n in enumerate(SIZES):
            ids = ids_pool[at:at + n].astype(np.uint32)
            at += n
            dead = rng.random(n) < 0.06  # delete marks: bit 31
            ids = np.where(dead, ids | np.uint32(0x80000000), ids).astype(
                np.uint32)
            self.lists.append((ids, kr.grid((n, d), seed=100 * d + li)))
        # exact duplicates across lists, under other ids
        self.lists[10][1][:] = self.lists[L[1100]][1][:9]
        self.lists[11][1][:64] = self.lists[L[129]][1][:64]
        self.lists[L[8]][1][:4] = self.lists[L[1100]][1][500:504]
        self.deleted = rng.random(NDOC) < 0.10  # the bitmap
        self._want = {}

    def expect(self, name, k2, ip, bitmap):
        if (name, ip, bitmap) not in self._want:
            rows = []
            for qi, probes in enumerate(TABLES[name]):
                dist, ids = [np.empty(0, np.float32)], [np.empty(0, np.int64)]
                for ln in probes:
                    if ln < 0 or ln >= NLIST or SIZES[ln] == 0:
                        continue
                    lid, vecs = self.lists[ln]
                    q = self.queries[qi:qi + 1]
                    dd = (kr.dots_exact(q, vecs) if ip
                          else kr.l2_exact(q, vecs))[0]
                    live = (lid >> 31) == 0
                    dist.append(dd[live])
                    ids.append(lid[live].astype(np.int64))
                rows.append((np.concatenate(dist), np.concatenate(ids)))
            self._want[(name, ip, bitmap)] = rows
        return np.stack([
            kr.topk_keys(dist, ids, k2, ip,
                         deleted=self.deleted if bitmap else None)
            for dist, ids in self._want[(name, ip, bitmap)]])

    def run(self, name, k2, ip, bitmap):
        from vearch_amd import ktest
        t = TABLES[name]
        return ktest.ivfflat_scan(
            self.lists, t, self.queries[:t.shape[0]], k2, ip,
            bitmap=kr.bitmap_words(self.deleted) if bitmap else None)


_cases = {}


def _case(d):
    if d not in _cases:
        _cases[d] = Case(d)
    return _cases[d]


@pytest.mark.parametrize("bitmap", [False, True], ids=["nobitmap", "bitmap"])
@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("d", DIMS)
def test_ivfflat_scan_rows(d, ip, bitmap):
    c = _case(d)
    for name in TABLES:
        for k2 in (1, 10, 300, 1024):
            got = c.run(name, k2, ip, bitmap)
            want = c.expect(name, k2, ip, bitmap)
            assert np.array_equal(got, want), (name, d, ip, bitmap, k2)


def test_ivfflat_case_has_what_the_kernel_can_get_wrong():
    """The fixture itself: a row with more than 1024 live candidates under
    the bitmap (so k2 = 1024 selects), delete marks present, and equal
    distances under different ids inside the top 300 (so ties are
    decided)."""
    c = _case(36)
    want = c.expect("rows5", 1024, False, True)
    assert (want[0] != kr._EMPTY).all()
    assert any((ids >> 31).any() for ids, _ in c.lists)
    d300, i300 = kr.key_decode(c.expect("rows5", 300, False, False)[3],
                               False)
    assert len(set(i300.tolist())) == 300
    assert len(np.unique(d300)) < 300
