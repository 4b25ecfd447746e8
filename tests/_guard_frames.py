"""Child process of tests/test_own_surface_roots.py: renders the named golden snapshots with whatever library QR_LIB selects
(the guarded diagnostic build) and prints `name hash` per snapshot, FNV-1a-64 as in tests/golden/manifest.json."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    from conftest import load_blob
    from qr_loader import load_package
    qr = load_package()
    for name in sys.argv[1:]:
        scn = qr.Scene(load_blob(name))
        frame = scn.new_frame()
        scn.render(frame)
        scn.render_count()                      # the guarded build reports bad cell offsets here (stderr)
        torch.cuda.synchronize()
        print(name, "%016x" % qr.frame_hash(frame), flush=True)
        scn.close()


if __name__ == "__main__":
    main()
