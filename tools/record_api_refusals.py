#!/usr/bin/env python3
"""Record what the ray API's entry points answer to the bad calls of tests/_api_refusals.py: tests/golden/api_refusals.json,
which tests/test_api_refusals.py holds every later build to.

Run it with the library of the commit that is to be the reference (the parent of a change to the host glue), never with
the build under test:

    python tools/record_api_refusals.py --parent <commit hash of the library's source> [--recording NAME] [--out FILE]

--recording: which file of tests/_api_refusals.py RECORDINGS, with its functions (default: the first, api_refusals.json).

The file holds the table of distinct (status, message) outcomes and, per fixture and function, one outcome index per case
in the table's order, with a digest of the case ids so that a changed table is noticed.
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
    ap.add_argument("--parent", required=True, help="commit hash of the source the loaded library was built from")
    ap.add_argument("--recording", default="api_refusals.json")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import _api_refusals as A
    functions = A.RECORDINGS[args.recording]
    args.out = args.out or os.path.join(ROOT, "tests", "golden", args.recording)
    import qr_oracle
    from conftest import load_blob
    from qr_loader import load_package
    qr = load_package()

    outcomes, results = {}, {}

    def visit(fixture, name, cid, got):
        results.setdefault(fixture, {}).setdefault(name, []).append(outcomes.setdefault(got, len(outcomes)))

    rigs = A.open_rigs(qr, load_blob)
    A.run(rigs, visit, functions)   # stops at the first case that was not refused before the device
    ids, ref = A.survivor_trace(rigs[A.FIXTURES[0]], qr_oracle, load_blob(A.FIXTURES[0]))
    if not (ids == ref).all():
        raise SystemExit("the scene does not trace as the oracle does after the refused calls")
    for r in rigs.values():
        r.close()

    doc = {"parent": args.parent, "library": qr.lib().qr_version().decode(),
           "outcomes": [list(o) for o, _ in sorted(outcomes.items(), key=lambda kv: kv[1])],
           "digest": {f["name"]: A.table_digest(f) for f in functions},
           "results": results}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    n = sum(len(v) for fx in results.values() for v in fx.values())
    print(f"{n} cases, {len(outcomes)} distinct outcomes -> {args.out}")


if __name__ == "__main__":
    main()
