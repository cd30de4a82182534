"""The refusals the six aggregation calls on resident ciphertexts share (csrc/capi_aggregate.inc: agg_admit) and one
parameter refusal of each call's own, under a 1024- and a 2048-bit key: the return code and the FULL text of
pgpu_last_error() against tests/golden/aggregate_refusals.json, `*out` left null, and no launch at all
(pgpu_timing_collect_ex reports none).  The fixture was recorded by tests/golden/gen_aggregate_refusals.py at the commit
before the six host drivers were folded into one, and the cases are driven by that generator's collect(): the C API
alone, so the test passes on either side of that change -- it is what holds the shared admission tail to the messages,
codes and order of the six separate ones (matvec's odd "ciphertext batch belongs to a different key" included).
Every case violates exactly one condition; operands are 2-6 ciphertexts and nothing is exponentiated."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
_spec = importlib.util.spec_from_file_location("gen_aggregate_refusals", os.path.join(GOLD, "gen_aggregate_refusals.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)
_results = {}


def results(engine, bits, other_n):
    if bits not in _results:     # one pass over all calls and cases per key, shared by the tests below
        _results[bits] = gen.collect(engine, bits, other_n)
    return _results[bits]


@pytest.mark.parametrize("op", gen.OPS)
@pytest.mark.parametrize("bits", [1024, 2048])
def test_refusal_codes_and_messages(engine, bits, op):
    want = json.load(open(os.path.join(GOLD, "aggregate_refusals.json")))
    got = results(engine, bits, int(want["other_n"][str(bits)], 16))[op]
    assert set(got) == set(gen.CASES) | {"no_pair"}
    for case, r in got.items():
        rc, error = want["4096"][op] if case == "no_pair" else want[str(bits)][op][case]
        print(bits, op, case, r)
        assert rc != 0 and (r["rc"], r["error"]) == (rc, error), (bits, op, case)
        assert r["out_null"], (bits, op, case)
        assert r["launches"] == 0, (bits, op, case)
