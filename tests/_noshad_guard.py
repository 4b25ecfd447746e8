"""Child process of tests/test_noshad_walks.py, beside tests/_guard_frames.py: renders the named cases of its FRAME_CASES (a scene
of tests/_noshad.py, the environment at upload, tile binning) with whatever library QR_LIB selects -- the guarded diagnostic
build -- and prints `case hash` per case, FNV-1a-64 as in tests/golden/manifest.json."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    import _noshad as N
    from qr_loader import load_package
    from test_noshad_walks import FRAME_CASES
    qr = load_package()
    for case in sys.argv[1:]:
        scene, e, rebin = FRAME_CASES[case]
        with N.env(e):
            scn = qr.Scene(N.scene_blob(scene), rebin_tiles=rebin)
        frame = scn.new_frame()
        scn.render(frame)
        scn.render_count()                      # the guarded build reports bad cell offsets here (stderr)
        torch.cuda.synchronize()
        print(case, "%016x" % qr.frame_hash(frame), flush=True)
        scn.close()


if __name__ == "__main__":
    main()
