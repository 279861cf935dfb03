"""CPU-side checks of the C-ABI library: it builds, loads without a GPU, exports every
symbol include/annchor_hip.h declares, and fails loudly (no fallback) without a device."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as g

    g.build()
    from annchor_amd import _native

    return _native


def _declared():
    hdr = open(os.path.join(ROOT, "include", "annchor_hip.h")).read()
    return sorted(set(re.findall(r"\b(annchor_[a-z0-9_]+)\s*\(", hdr)))


def test_header_and_binding_agree(native):
    assert _declared() == native.exported_symbols()


def test_library_exports_every_declared_symbol(native):
    lib = native.load_library()
    for name in _declared():
        assert hasattr(lib, name), name


def test_no_silent_fallback_without_gpu(native):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(native.NativeError, match="no CPU fallback"):
        native.Engine(0)
    from annchor_amd import Annchor

    with pytest.raises(native.NativeError):
        Annchor(["abc", "abd", "xyz"], "levenshtein")


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "annchor_amd")
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, fn)).read()
                assert "oracle" not in txt.replace("no CPU oracle", ""), os.path.join(dirpath, fn)


def _env_table():
    """Variables named in the first column of INTEGRATION.md's "Environment switches" table."""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = doc[doc.index("## Environment switches"):]
    nxt = sec.find("\n## ", 1)
    sec = sec if nxt < 0 else sec[:nxt]
    names = set()
    for line in sec.splitlines():
        if line.startswith("| `"):
            names.update(re.findall(r"`(ANNCHOR_[A-Z0-9_]+)", line.split(" | ")[0]))
    return names


def _sources(roots, exts):
    for root in roots:
        path = os.path.join(ROOT, root)
        if os.path.isfile(path):
            yield path
            continue
        for dirpath, _, files in os.walk(path):
            for fn in files:
                if fn.endswith(exts):
                    yield os.path.join(dirpath, fn)


def test_environment_table_matches_the_code():
    """Every ANNCHOR_* variable the library reads has a row in INTEGRATION.md's Environment table, and every variable
    there is still read by the library, bench.py or a tool."""
    table = _env_table()
    read = set()
    for path in _sources(["annchor_amd/csrc"], (".hip", ".h", ".cpp")):
        read.update(re.findall(r'getenv\("(ANNCHOR_[A-Z0-9_]+)"', open(path).read()))
    pkg = os.path.join(ROOT, "annchor_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            read.update(re.findall(r'environ(?:\.get\(|\[)"(ANNCHOR_[A-Z0-9_]+)"', open(os.path.join(pkg, fn)).read()))
    assert read, "no environment reads found"
    assert sorted(read - table) == [], "read by the library but missing from INTEGRATION.md's Environment table"
    used = set()
    for path in _sources(["annchor_amd", "bench.py", "tools"], (".py", ".hip", ".h", ".cpp", ".sh")):
        used.update(re.findall(r"ANNCHOR_[A-Z0-9_]+", open(path, errors="replace").read()))
    assert sorted(table - used) == [], "listed in INTEGRATION.md's Environment table but read nowhere"
