"""Regenerates tests/golden/reference_*.npz: recorded results of the compiled reference (oracle/_ref/nbody_ref — the reference's own
OctreeSearch.cpp under g++ against oracle/ue4_standin/; `make -C oracle reference`).  Data only: inputs, and what the program wrote.
Layout and scenes: tests/reference_scenes.py.  Needs the reference's sources (or a built oracle/_ref/nbody_ref); no GPU.

    python tests/golden/make_reference_golden.py [--new-inputs]

Without --new-inputs the small scenes keep the inputs already committed (records0) and only the outputs are recorded again.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import reference_scenes as S            # noqa: E402
from oracle import oracle as O          # noqa: E402
from oracle import reference as R       # noqa: E402

if __name__ == "__main__":
    O.build()
    assert R.build() is not None, "no oracle/_ref/nbody_ref and no reference sources at " + R.reference_dir()
    new_inputs = "--new-inputs" in sys.argv[1:]
    for name in S.NAMES:
        path = os.path.join(HERE, S.file_name(name))
        stored = name == "forces_theta0" or (not new_inputs and os.path.exists(path))   # (forces: the scene files just written)
        arrays = S.record(name, R, O, stored_inputs=stored)
        np.savez_compressed(path, **arrays)
        print(S.file_name(name), os.path.getsize(path), "bytes", {k: v.shape for k, v in arrays.items()})
