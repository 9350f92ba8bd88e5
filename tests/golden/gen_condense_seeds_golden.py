"""Records tests/golden/condense_seeds_golden.npz for
tests/test_sens_condense_bitwise.py::test_condensing_seeds_bitwise_vs_recorded
(needs the GPU).  The library is the one KITE_NMPC_LIB names: record with the
build whose condensed QPs are to be kept.  Two kites, N = 20, one cold and one
warm step (run_seed_case):
  kite 0  the warm step is linearised around a planted plan whose dE is exactly
          at its upper bound at interval 6 and whose dR is exactly at its lower
          bound at interval 9;
  kite 1  the angular rate wy of the measured state is exactly 0.0 in both
          steps (a signed-zero probe for the propagation's seeds).
Stored: the inputs (x0, x1, the planted plan) and H, h, C of both kites after
each step, as kite_nmpc_get_qp returns them.
  python tests/golden/gen_condense_seeds_golden.py [OUT.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_sens_condense_bitwise import run_seed_case, seed_inputs  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "condense_seeds_golden.npz")
    np.savez_compressed(out, **run_seed_case(seed_inputs()))
    print("wrote", out, os.path.getsize(out), "bytes")
