"""What the query entries refuse before any device is touched, whole: every case of tools/record_query_refusals.py replayed against both
built libraries, status and rt_last_error_message() compared exactly with tests/golden/query_refusals.json -- the table that tool recorded
before the launch layer's checks were folded into shared pieces (NOTES.md).  The per-query host tests hold the same refusals by substring;
this one holds their text, their order and the f64 stand-in.  No GPU: a stand-in scene handle, as in tests/test_sweep_host.py."""
import ctypes
import importlib.util
import json
import os

import pytest

from rust_tracer_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recorder():
    spec = importlib.util.spec_from_file_location("record_query_refusals", os.path.join(ROOT, "tools", "record_query_refusals.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("path", [capi.PRODUCT_LIB_PATH, capi.TEST_LIB_PATH], ids=["product", "test_hooks"])
def test_every_recorded_refusal_is_made_with_the_same_status_and_message(path):
    recorder = _recorder()
    with open(recorder.TABLE) as f:
        table = json.load(f)
    lib = ctypes.CDLL(path)
    cases = list(recorder.cases())
    assert sorted(c.id for c in cases) == sorted(table) and len(table) > 900
    # every query entry, host and device, in both precisions
    assert {c.id.split("/")[0] for c in cases} == {n for n in capi.SYMBOLS if n in recorder.ENTRIES} and len(recorder.ENTRIES) == 28
    differing = {}
    for c in cases:
        got = list(c.run(lib))
        if got != table[c.id]:
            differing[c.id] = (got, table[c.id])
    assert not differing, differing
