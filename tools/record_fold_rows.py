#!/usr/bin/env python3
"""Record tests/golden/fold_rows_digest.npz: one sha256 per board of k_embed_fold's rows (bf16 kernel and its float32 EX form) over
the board sets of tests/fold_bits_common.py, default grid.  Run it on an MI355X with the build whose rows are the reference - the
parent of a change that must keep the rows bit for bit - and commit the file; tests/test_gpu_fold_bits.py holds every later build
to it.
    python tools/record_fold_rows.py [out.npz]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "alpha-zero_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

import fold_bits_common as fb  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "fold_rows_digest.npz")
    rec = {}
    for name in fb.CONFIGS:
        boards, labels = fb.board_set(name)
        for exact in (False, True):
            tables = fb.fold_tables(name, exact)
            rows, sched = fb.run_rows(name, boards, tables, exact)
            assert sched == [0, 0], sched
            again, _ = fb.run_rows(name, boards, tables, exact, grid=2)
            assert np.array_equal(rows.view(np.uint8), again.view(np.uint8)), "the recording build is not schedule-independent"
            rec[fb.key(name, exact)] = fb.digests(rows)
            print(fb.key(name, exact), len(labels), "boards", rec[fb.key(name, exact)][0][:16])
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
