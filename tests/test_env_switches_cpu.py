"""CPU: the environment variables the C++/HIP engine reads are exactly the ones INTEGRATION.md lists under "Environment
variables" (minus HMOGP_LIB_PATH, which the Python binding reads).  The list is single-sourced, and a new switch in the
engine is a visible decision: it fails here until it is documented."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hetmogp_amd", "csrc")
HELPER = "env_num"          # common.h: the one function that calls getenv


def read_by_engine():
    names, stray = set(), []
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if not os.path.isfile(path):
            continue
        src = open(path, errors="replace").read()
        names.update(re.findall(r"\b(?:getenv|%s)\s*\(\s*\"(HMOGP_[A-Z0-9_]+)\"" % HELPER, src))
        # a getenv whose argument is not an HMOGP_ literal would escape the collection above: only the helper's own may be one
        for m in re.finditer(r"\bgetenv\s*\(\s*([^)]*)\)", src):
            if not re.match(r"\"HMOGP_[A-Z0-9_]+\"\s*$", m.group(1)):
                stray.append((os.path.basename(path), m.group(0)))
    return names, stray


def documented():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"^#+ Environment variables\s*$", doc, flags=re.M)
    assert m, "INTEGRATION.md has no 'Environment variables' section"
    section = re.split(r"^#+ ", doc[m.end():], flags=re.M)[0]
    items = re.findall(r"^- `(HMOGP_[A-Z0-9_]+)`", section, flags=re.M)
    assert len(items) == len(set(items)), items
    return set(items)


def test_engine_reads_exactly_the_documented_environment_variables():
    names, stray = read_by_engine()
    assert stray == [("common.h", "getenv(name)")], stray
    doc = documented()
    assert "HMOGP_LIB_PATH" in doc
    assert names == doc - {"HMOGP_LIB_PATH"}, (sorted(names), sorted(doc))
    assert "HMOGP_LIB_PATH" in open(os.path.join(ROOT, "hetmogp_amd", "_lib.py")).read()
