"""Record tests/golden/net_walk_parent.npz: what gnnb_net_eval, gnnb_net_descend and gnnb_net_descend_starts compute on the cases of
tests/test_gpu_net_walk_parent.py, by the library BEFORE the scalar and the S-wide walk of the bound network became one template (run once,
on the GPU box):

    tools/mklib.sh <parent revision> parent
    GNNB_LIB=tools/ablate/parent.so python tools/net_walk_record.py [out.npz]

Per case the digests of its inputs are recorded beside the results; the test asserts them first."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tests import test_gpu_net_walk_parent as T              # noqa: E402
from tests.common import register_kw_archs, register_toy_archs      # noqa: E402


def main():
    from gnn_branching_amd.engine import ScorerEngine
    out = sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE
    register_kw_archs()
    register_toy_archs()
    engine, rec = ScorerEngine(None), {}
    for name in T.NETS:
        for B in T.BS:
            for what, d in T.input_digests(name, B).items():
                rec[f"{name}/B{B}/inputs/{what}"] = np.array(d)
            run = T.run_case(engine, name, B)
            again = T.run_case(engine, name, B)
            assert all(T.same_bits(run[k], again[k]) for k in run), (name, B, "two runs of the recorded library differ")
            for k, v in run.items():
                rec[f"{name}/B{B}/{k}"] = v
            print(f"{name} B {B}: eval {run['eval'].tolist()}, steps at (8, 1/2) {run['descend3/steps'].tolist()}, "
                  f"winners of 9 starts {run['starts9/index'].tolist()}")
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes; library:", os.environ.get("GNNB_LIB", "in-tree"))


if __name__ == "__main__":
    main()
