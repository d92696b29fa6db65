"""Record tests/golden/blocktap_parent.npz: scores, decisions and the row signatures of layer 1 after the first forward half-pass, for the
cases of tests/test_gpu_blocktap.py, computed by the library BEFORE the block form of the edge-1 forward tiles (run once, on the GPU box):

    tools/mklib.sh <parent revision> parent
    GNNB_LIB=tools/ablate/parent.so python tools/blocktap_record.py [out.npz]

The fused and the two-kernel half-pass of that library must agree bit for bit (the script checks it); both are recorded."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tests import test_gpu_blocktap as T      # noqa: E402
from tests.common import FAMILIES             # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE
    rec = {}
    for name in T.CASES:
        for fam in FAMILIES:
            runs = {path: T.run_case(name, fam, opts) for path, opts in T.PATHS.items()}
            for what in ("scores", "decisions", "row_sig"):
                assert np.array_equal(runs["default"][what], runs["fuse0"][what]), (name, fam, what)
            for path, r in runs.items():
                for what, v in r.items():
                    rec[f"{name}/{fam}/{path}/{what}"] = v
            print(f"{name} {fam}: scores {runs['default']['scores'].shape}, decisions {runs['default']['decisions'].tolist()}")
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes; library:", os.environ.get("GNNB_LIB", "in-tree"))


if __name__ == "__main__":
    main()
