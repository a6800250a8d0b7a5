#!/usr/bin/env python3
"""Record what the REFERENCE codec returns at every (k, m) of the library's domain into
tests/golden/ref_domain.json, so that tests/test_oracle_domain.py pins the CPU oracle to it
also where oracle/_ref cannot be built.  Needs oracle/_ref/libref_cauchy.so
(`make -C oracle ref`).  The committed output is pure data: the parameters of the sweep and
SHA-256 folds, one per m over that m's pairs in ascending k and one per k over that k's pairs
in ascending m.  Each pair's digest covers the encode return code, the parity bytes, the decode
status words, the row tags after the decode and the decoded blocks.  Inputs are not stored:
they come from quic_amd.synth and numpy by (k, m), as in the test.

Usage:  python tests/golden/gen_ref_domain.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import oracle as O  # noqa: E402
from tests import test_oracle_domain as D  # noqa: E402


def main():
    if not O.ref_available():
        sys.exit("needs oracle/_ref/libref_cauchy.so: run `make -C oracle ref` first")
    by_m = {str(m): D.fold_m(O, m, use_ref=True) for m in D.M_ALL}
    by_k = {str(k): D.fold_k(O, k, use_ref=True) for k in D.M_ALL}
    rec = dict(
        generator="tests/golden/gen_ref_domain.py",
        reference="net/quic/core/libcat/cauchy_256.cpp (compiled by oracle/Makefile)",
        block_bytes=D.BB, groups=D.GROUPS, seed_base=D.SEED,
        pairs=sum(len(D.ks_of(m)) for m in D.M_ALL),
        by_m=by_m, by_k=by_k)
    with open(os.path.join(HERE, "ref_domain.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(f"{rec['pairs']} pairs folded into {len(by_m)} + {len(by_k)} digests")


if __name__ == "__main__":
    main()
