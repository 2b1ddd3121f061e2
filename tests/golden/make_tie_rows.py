"""Writes tests/golden/tie_rows.npz: for the rows of one magnitude of tests/tie_numpy.py (TIE_CODES; the rows themselves are
regenerated from the oracle's channel by tie_numpy.tie_rows) and every list size the tests use, the indices of the EXACTLY
DECIDED rows (tie_numpy.walk with the "exact" arithmetic) and the oracle's decoded bits of all rows, packed. The oracle and the
model alone: no device is involved. Run from the repository root:

    python tests/golden/make_tie_rows.py

A row on which the model's word differs from the oracle's stops the run; tests/test_tie_model.py recomputes the arrays."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import tie_numpy as T  # noqa: E402


def main():
    out = {}
    for code, (rows, Ls) in T.TIE_CODES.items():
        o, c, x = T.case(code)
        for L in Ls:
            want = o.decode_scl_llr(x, L)
            exact = []
            for r in range(rows):
                res = T.walked(code, L, r)
                assert (res.info == want[r]).all(), (code, L, r)
                if res.exactly_decided():
                    exact.append(r)
            print(code, "L = %d: %d of %d rows exactly decided" % (L, len(exact), rows), exact)
            assert 2 * len(exact) >= rows
            out["exact_" + T.golden_key(code, L)] = np.asarray(exact, np.int32)
            out["bits_" + T.golden_key(code, L)] = np.packbits(want, axis=1)
    np.savez_compressed(T.GOLDEN_FILE, **out)
    print(T.GOLDEN_FILE, os.path.getsize(T.GOLDEN_FILE), "bytes")


if __name__ == "__main__":
    main()
