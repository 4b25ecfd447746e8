"""The refusals of the ray API's entry points at the C level, qr_trace_rays_async .. qr_layer_views_async and the image filters
qr_atrous_views_async, qr_upsample_views_async, qr_reproject_views_async and qr_reproject_moving_async: status and message text
of every single bad argument each function checks, and of every pair of them, which pins the order of the checks (tests/_api_refusals.py holds the table).

tests/golden/api_refusals.json, and api_refusals_filters.json for the filters that came after it, are what the commit named in
each answered (tools/record_api_refusals.py, run with that commit's library): the host glue in front of the kernels may be rearranged, what a caller is told may not change.
No case launches a kernel; the last step traces 64 rays on a scene that took every refused call."""
import json
import os

import pytest

import _api_refusals as A
from conftest import GOLDEN, load_blob


def _recordings():
    """(recording, its functions) of every file, the digest of the case table checked"""
    for name, functions in A.RECORDINGS.items():
        with open(os.path.join(GOLDEN, name)) as f:
            doc = json.load(f)
        assert doc["digest"] == {f["name"]: A.table_digest(f) for f in functions}, f"{name}: the case table changed: record again on the parent"
        yield doc, functions


def test_table_matches_the_recording():
    for doc, _ in _recordings():
        assert sorted(doc["results"]) == sorted(A.FIXTURES)
    assert sum(len(functions) for functions in A.RECORDINGS.values()) == len(A.FUNCTIONS)


@pytest.mark.gpu
def test_gpu_refusals_equal_the_parents(qr, oracle):
    rigs = A.open_rigs(qr, load_blob)
    try:
        for doc, functions in _recordings():
            outcomes = [tuple(o) for o in doc["outcomes"]]
            at, seen = {}, [0]

            def visit(fixture, name, cid, got):
                i = at[fixture, name] = at.get((fixture, name), -1) + 1
                want = outcomes[doc["results"][fixture][name][i]]
                assert got == want, f"{fixture} {name} {cid}: got {got}, the parent ({doc['parent'][:12]}) answered {want}"
                seen[0] += 1

            A.run(rigs, visit, functions)
            assert seen[0] == sum(len(v) for fx in doc["results"].values() for v in fx.values())
        ids, ref = A.survivor_trace(rigs[A.FIXTURES[0]], oracle, load_blob(A.FIXTURES[0]))
        assert (ids == ref).all()
    finally:
        for r in rigs.values():
            r.close()
