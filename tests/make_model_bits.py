"""Writes tests/golden/model_bits.npz: what the build found on sys.path gives on the cases of model_bits_cases.py, on the GPU.

    python tests/make_model_bits.py OUT.npz COMMIT [ROOT]

COMMIT is the hash of the commit whose build is recorded (stored in the fixture as `commit`); ROOT is the checkout whose
annchor_amd package is driven (default: this file's repository).  The fixture in the tree was recorded on an MI355X from the
commit BEFORE the model kernels moved their work matrix and their sort keys into LDS and registers, so that
test_model_kernels_bits_gpu.py pins the later kernels to that build's bits."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main(out, commit, root=os.path.dirname(HERE)):
    sys.path.insert(0, os.path.abspath(root))
    sys.path.insert(0, HERE)
    import annchor_amd
    import model_bits_cases as B
    print("recording %s of %s" % (commit, os.path.dirname(os.path.abspath(annchor_amd.__file__))))
    D = B.Driver()
    rec = {"commit": np.array(commit), "cases": np.array(B.CASES)}
    try:
        for name in B.CASES:
            r = D.run(name)
            print("  %-18s m %6d nb %2d longest list %5d flags %s" % (name, r["shape"][0], r["shape"][1], r["shape"][2], r["flags"]))
            for k, v in r.items():
                rec["%s/%s" % (name, k)] = v
    finally:
        D.close()
    np.savez_compressed(out, **rec)
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main(*sys.argv[1:4])
