#!/usr/bin/env python3
"""Record what the REFERENCE codec returns for the cases that tests/test_oracle_golden.py and
tests/test_loopback.py compare against the compiled reference, into
tests/golden/ref_recorded.json, so that those tests also run where oracle/_ref cannot be
built.  Needs oracle/_ref/libref_cauchy.so (`make -C oracle ref`) and the loopback tool
(`make tools`).  The committed output is pure data: return codes, status words, the loopback
tool's counters and SHA-256 digests of the output buffers and row fields.  Inputs are not
stored: they come from quic_amd.synth by seed, as in the tests.

Usage:  python tests/golden/gen_ref_recorded.py
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import oracle as O  # noqa: E402
from quic_amd import synth  # noqa: E402
from tests.test_loopback import CASES, REF_LIB, TOOL  # noqa: E402
from tests.test_oracle_golden import REF_CASES, REF_GROUPS  # noqa: E402


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def direct(k, m, bb, r):
    data = synth.group_data(99 + k, k, bb, REF_GROUPS)
    par, rc = O.encode_batch(k, m, bb, data, use_ref=True)
    rows, src = synth.loss_patterns(k, m, r, REF_GROUPS, 5, shuffle=True)
    recv = synth.assemble_received(data, par, src)
    blocks, rows_out, status = O.decode_batch(k, m, bb, recv, rows, use_ref=True)
    return dict(encode_rc=int(rc), parity_sha256=sha(par), blocks_sha256=sha(blocks),
                rows_sha256=sha(rows_out), status=status.tolist())


def loopback(args):
    cmd = [TOOL, "--fec", *args, f"--cpu-codec={REF_LIB}",
           f"--tables={ROOT}/quic_amd/data/cauchy_256_tables.bin"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=ROOT)
    d = json.loads(out.stdout.strip().splitlines()[-1])
    return {key: d[key] for key in ("dropped", "revived", "unrecovered", "sha256_out")}


def main():
    if not (O.ref_available() and os.path.exists(TOOL)):
        sys.exit("needs oracle/_ref/libref_cauchy.so and quic_amd/bin/fec_loopback: "
                 "run `make -C oracle ref` and `make tools` first")
    rec = dict(
        generator="tests/golden/gen_ref_recorded.py",
        reference="net/quic/core/libcat/cauchy_256.cpp (compiled by oracle/Makefile)",
        direct={"_".join(map(str, c)): direct(*c) for c in REF_CASES},
        loopback={" ".join(a): loopback(a) for a in CASES})
    with open(os.path.join(HERE, "ref_recorded.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(f"{len(rec['direct'])} direct and {len(rec['loopback'])} loopback cases written")


if __name__ == "__main__":
    main()
