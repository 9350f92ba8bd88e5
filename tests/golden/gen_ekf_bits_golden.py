"""Records tests/golden/ekf_bits_golden.npz for
tests/test_ekf_bitwise.py::test_ekf_kernels_bitwise_vs_recorded (needs the GPU).
The library is the one KITE_NMPC_LIB names: record with the build whose filter
outputs are to be kept (the commit before the kernels' measurement update moved
into csrc/ekf_update.hpp).  Stored: the outputs of every case of
test_ekf_bitwise.run_cases (x and P as uint64 bits, the status words as int32);
the inputs are regenerated from the seed by test_ekf_bitwise.seeded_inputs.
  python tests/golden/gen_ekf_bits_golden.py [OUT.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_ekf_bitwise import run_cases  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "ekf_bits_golden.npz")
    got = run_cases()
    for k in sorted(got):
        if k.endswith("/st"):
            print(k, got[k].tolist())
    np.savez_compressed(out, **got)
    print("wrote", out, os.path.getsize(out), "bytes")
