"""Every gk:: entry of csrc/kernels.h has a kernel test hook, and every
hook has its ctypes signature declared. Source text only: no library is
loaded, so this runs where nothing is built."""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(REPO, *parts)) as f:
        return f.read()


def _strip_comments(src):
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    return re.sub(r"//[^\n]*", " ", src)


def _gk_entries():
    src = _strip_comments(_read("vearch_amd", "csrc", "kernels.h"))
    m = re.search(r"namespace\s+gk\s*\{(.*)\}", src, flags=re.S)
    assert m, "kernels.h has no namespace gk"
    return sorted(set(re.findall(r"\bhipError_t\s+(\w+)\s*\(", m.group(1))))


def _hooks():
    src = _strip_comments(_read("vearch_amd", "csrc", "ktest.cpp"))
    return src, sorted(set(re.findall(r"\bint\s+(GammaKTest\w+)\s*\(", src)))


def test_parser_sees_the_known_entries():
    names = _gk_entries()
    assert len(names) >= 30, names
    for known in ("ivfpq_scan", "ivfflat_scan", "bucket_scatter",
                  "pq_sterm_buckets", "rabitq_sval_buckets", "dots_mfma"):
        assert known in names
    _, hooks = _hooks()
    assert "GammaKTestIvfpqScan" in hooks and len(hooks) >= 30


def test_every_gk_entry_is_called_from_a_hook():
    src, _ = _hooks()
    missing = [n for n in _gk_entries()
               if not re.search(r"\bgk::%s\s*\(" % n, src)]
    assert not missing, f"gk:: entries without a kernel test hook: {missing}"


def test_every_hook_is_declared_and_typed():
    _, hooks = _hooks()
    header = _strip_comments(_read("include", "gamma_bench.h"))
    py = _read("vearch_amd", "ktest.py")
    undeclared = [h for h in hooks
                  if not re.search(r"\bint\s+%s\s*\(" % h, header)]
    assert not undeclared, f"hooks missing from gamma_bench.h: {undeclared}"
    untyped = [h for h in hooks
               if not re.search(r"\bL\.%s\.argtypes\s*=" % h, py)]
    assert not untyped, f"hooks without argtypes in ktest.py: {untyped}"
