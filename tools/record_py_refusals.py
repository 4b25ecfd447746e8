#!/usr/bin/env python3
"""Record what the Python binding answers to the bad calls of tests/_py_refusals.py: tests/golden/py_refusals.json, which
tests/test_py_refusals.py holds every later binding to.

Run it with the binding of the commit that is to be the reference (the parent of a change to quadray-engine_amd/__init__.py),
never with the binding under test:

    python tools/record_py_refusals.py --parent <commit hash of the binding> [--recording NAME] [--out FILE]

--recording: which file of tests/_py_refusals.py RECORDINGS, with its functions (default: the first, py_refusals.json).

The file holds the table of distinct (type name, text) outcomes and one outcome index per case in the table's order, with a
digest of the case ids so that a changed table is noticed.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="commit hash of the binding that is loaded")
    ap.add_argument("--recording", default="py_refusals.json")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import _api_refusals as A
    import _py_refusals as P
    functions = P.RECORDINGS[args.recording]
    args.out = args.out or os.path.join(ROOT, "tests", "golden", args.recording)
    import qr_oracle
    from conftest import load_blob
    from qr_loader import load_package
    qr = load_package()

    outcomes, results = {}, []
    rig = P.Rig(qr, load_blob(P.FIXTURE))
    P.run(rig, lambda name, cid, got: results.append(outcomes.setdefault(got, len(outcomes))), functions)   # stops at a case not refused
    ids, ref = A.survivor_trace(rig, qr_oracle, load_blob(P.FIXTURE))
    if not (ids == ref).all():
        raise SystemExit("the scene does not trace as the oracle does after the refused calls")
    rig.close()

    doc = {"parent": args.parent, "library": qr.lib().qr_version().decode(),
           "outcomes": [list(o) for o, _ in sorted(outcomes.items(), key=lambda kv: kv[1])],
           "digest": P.table_digest(functions), "results": results}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(results)} cases, {len(outcomes)} distinct outcomes -> {args.out}")


if __name__ == "__main__":
    main()
