"""The refusals of the ray API's entry points at the C level: status and message text of every single bad argument each
function checks, and of every pair of them, which pins the order of the checks (tests/_api_refusals.py holds the table).

tests/golden/api_refusals.json is what the commit named in it answered (tools/record_api_refusals.py, run with that
commit's library): the host glue in front of the kernels may be rearranged, what a caller is told may not change.
No case launches a kernel; the last step traces 64 rays on a scene that took every refused call."""
import json
import os

import pytest

import _api_refusals as A
from conftest import GOLDEN, load_blob


def test_table_matches_the_recording():
    with open(os.path.join(GOLDEN, "api_refusals.json")) as f:
        doc = json.load(f)
    assert doc["digest"] == {f["name"]: A.table_digest(f) for f in A.FUNCTIONS}
    assert sorted(doc["results"]) == sorted(A.FIXTURES)


@pytest.mark.gpu
def test_gpu_refusals_equal_the_parents(qr, oracle):
    with open(os.path.join(GOLDEN, "api_refusals.json")) as f:
        doc = json.load(f)
    assert doc["digest"] == {f["name"]: A.table_digest(f) for f in A.FUNCTIONS}, "the case table changed: record again on the parent"
    outcomes = [tuple(o) for o in doc["outcomes"]]
    at, seen = {}, [0]

    def visit(fixture, name, cid, got):
        i = at[fixture, name] = at.get((fixture, name), -1) + 1
        want = outcomes[doc["results"][fixture][name][i]]
        assert got == want, f"{fixture} {name} {cid}: got {got}, the parent ({doc['parent'][:12]}) answered {want}"
        seen[0] += 1

    rigs = A.open_rigs(qr, load_blob)
    try:
        A.run(rigs, visit)
        assert seen[0] == sum(len(v) for fx in doc["results"].values() for v in fx.values())
        ids, ref = A.survivor_trace(rigs[A.FIXTURES[0]], oracle, load_blob(A.FIXTURES[0]))
        assert (ids == ref).all()
    finally:
        for r in rigs.values():
            r.close()
