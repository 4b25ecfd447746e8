"""Node-tree fixtures (tests/golden/tree/<name>.json.gz: the reference engine's object hierarchy of a snapshot, floats as hex
words) as the package's node tables.  No pytest here: the tests and the GPU tools (tools/gpu_reproject_moving.py) both load
trees through this file; tests/test_hierarchy.py states the same reader for its own cases, and tests/test_reproject_moving.py
holds the two to each other."""
import gzip
import json
import os

import numpy as np

TREE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tree")


def _f32(words):
    return np.array([int(x, 16) for x in words], dtype=np.uint32).view(np.float32)


def nodes_from_tree(qr, t):
    """the `nodes` of a tree fixture as a qr.node_dtype() array"""
    nodes = np.zeros(len(t["nodes"]), dtype=qr.node_dtype())
    for i, n in enumerate(t["nodes"]):
        r = nodes[i]
        r["parent"], r["tag"] = n["parent"], n["tag"]
        r["scl"], r["rot"], r["pos"], r["shape"] = _f32(n["scl"]), _f32(n["rot"]), _f32(n["pos"]), _f32(n["shape"])
        r["srf"], r["inb"], r["bvb"], r["lgt"] = n.get("srf", -1), n.get("inb", -1), n.get("bvb", -1), n.get("lgt", -1)
        r["anim"] = -1
        r["bvnode"], r["nverts"] = n.get("bvnode", -1), n.get("verts_num", 0)
        if "lmin" in n:
            r["lmin"], r["lmax"] = _f32(n["lmin"]), _f32(n["lmax"])
        if "tex" in n:
            r["tex"], r["has_tex"] = _f32(n["tex"]), 1
        if "pov" in n:
            r["pov"] = _f32(n["pov"])[0]
    return nodes


def load_tree(qr, name):
    """(the fixture's dict -- `opts`, `camera`, `nodes` --, its node table)"""
    with open(os.path.join(TREE, name + ".json.gz"), "rb") as f:
        t = json.loads(gzip.decompress(f.read()))
    return t, nodes_from_tree(qr, t)
