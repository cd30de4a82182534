"""The drop-in claim of INTEGRATION.md, checked: the reference's OWN client sources -- test/*.cpp, benchmark/*.cpp,
example/*.cpp -- parse and type-check UNCHANGED against include/ipcl (our mirror of the public ipcl:: API:
KeyPair / PublicKey / PrivateKey / PlainText / CipherText / BigNumber, ipcl/include/ipcl/*.hpp).

The sources are never copied into this repository: build() compiles them where they lie in the reference tree
(oracle/ref_dropin.py; googletest / google-benchmark replaced by the two stand-in headers under tests/cpp/shims) and
records the outcome in oracle/_ref/dropin.json.  This test reads that record only; the cases are the committed list of
names in tests/golden/dropin_sources.json.  Skips when build() had no reference tree to compile from."""
import json
import os

import pytest

from oracle import ref_dropin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = json.load(open(os.path.join(ROOT, "tests", "golden", "dropin_sources.json")))["sources"]


def _record():
    if not os.path.exists(ref_dropin.RECORD):
        pytest.skip("no oracle/_ref/dropin.json: build() had no reference tree to compile the client sources from")
    with open(ref_dropin.RECORD) as f:
        rec = json.load(f)
    assert rec["headers_sha256"] == ref_dropin.header_digest(), \
        "oracle/_ref/dropin.json was made against other headers than include/ipcl as it stands: run build()"
    return rec


@pytest.mark.parametrize("src", SOURCES)
def test_reference_client_source_compiles_unchanged(src):
    r = _record()["results"].get(src)
    assert r is not None, "%s is not among the client sources build() compiled" % src
    assert r["returncode"] == 0, "%s does not compile against include/ipcl:\n%s" % (src, r["stderr"])


def test_the_check_covers_every_client_source():
    rec = _record()
    assert len(SOURCES) >= 11, SOURCES
    assert rec["found"] == SOURCES, "the reference's client sources and tests/golden/dropin_sources.json differ"
