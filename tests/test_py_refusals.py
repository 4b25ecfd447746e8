"""The refusals of the Python binding: exception type and text of every single bad argument that Scene's ray API methods
(trace .. render_views_mean, atrous, denoise, upsample, reproject), the four accumulators and Temporal refuse (themselves, or the library behind them), and of every pair of them, which pins the order of
the checks (tests/_py_refusals.py holds the table; test_api_refusals.py is the same one layer down).

tests/golden/py_refusals.json, and py_refusals_filters.json for what came after it, are what the binding of the commit named in
each answered (tools/record_py_refusals.py, run with that commit's binding): the glue in quadray-engine_amd/__init__.py may be rearranged, what a caller is told may not change.
No case launches a kernel; the last step traces 64 rays on the scene that took every refused call."""
import json
import os

import pytest

import _api_refusals as A
import _py_refusals as P
from conftest import GOLDEN, load_blob


def _recordings():
    """(recording, its functions) of every file, the digest of the case table checked"""
    for name, functions in P.RECORDINGS.items():
        with open(os.path.join(GOLDEN, name)) as f:
            doc = json.load(f)
        assert doc["digest"] == P.table_digest(functions), f"{name}: the case table changed: record again with the parent's binding"
        yield doc, functions


def test_table_matches_the_recording():
    for doc, functions in _recordings():
        assert len(doc["results"]) == sum(len(P.cases(f)) for f in functions)
    assert sum(len(functions) for functions in P.RECORDINGS.values()) == len(P.FUNCTIONS)


@pytest.mark.gpu
def test_gpu_refusals_equal_the_parents(qr, oracle):
    rig = P.Rig(qr, load_blob(P.FIXTURE))
    try:
        for doc, functions in _recordings():
            outcomes = [tuple(o) for o in doc["outcomes"]]
            seen = [0]

            def visit(name, cid, got):
                want = outcomes[doc["results"][seen[0]]]
                assert got == want, f"{name} {cid}: got {got}, the parent ({doc['parent'][:12]}) answered {want}"
                seen[0] += 1

            P.run(rig, visit, functions)
            assert seen[0] == len(doc["results"])
        ids, ref = A.survivor_trace(rig, oracle, load_blob(P.FIXTURE))
        assert (ids == ref).all()
    finally:
        rig.close()
