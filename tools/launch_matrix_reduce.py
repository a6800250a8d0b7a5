#!/usr/bin/env python3
"""Fold one run of tools/launch_matrix.py into text small enough to keep and to diff.

    python3 tools/launch_matrix_reduce.py calls.txt run_kernel_trace.csv > reduced.txt

calls.txt is the driver's output, the CSV the rocprofv3 kernel trace of the same run.  Each
call's printed line gets the library's kernels the device ran for it, in dispatch order:
demangled name up to its template arguments, grid in work-items, workgroup size, LDS bytes
(the tracer reports static LDS only).  Calls of one shape that printed and ran the same are
listed once, under their call kinds, group counts, pointer offsets and option sets (numbered
at the top).
"""
import csv
import sys


def short(name):
    """`void qfec::f<...>(args)` -> `f<...>`."""
    name = name.replace("void ", "", 1).replace("(anonymous namespace)::", "")
    depth = 0
    for i, ch in enumerate(name):
        depth += (ch == "<") - (ch == ">")
        if ch == "(" and depth == 0:
            name = name[:i]
            break
    return name.replace("qfec::", "")


def ranges(ns):
    """[0, 1, 2, 5] -> "0-2,5"."""
    out = []
    for n in sorted(ns):
        if out and out[-1][1] == n - 1:
            out[-1][1] = n
        else:
            out.append([n, n])
    return ",".join(str(a) if a == b else "%d-%d" % (a, b) for a, b in out)


def main(calls_path, trace_path):
    with open(trace_path, newline="") as fh:
        rows = sorted(csv.DictReader(fh), key=lambda r: (int(r["Start_Timestamp"]), int(r["Dispatch_Id"])))
    runs, inside = [], False   # one run of the library's kernels per call
    for r in rows:
        if r["Kernel_Name"].startswith("__amd_rocclr_"):
            continue   # the runtime's own copy / fill kernels inside a host form
        if "qfec" not in r["Kernel_Name"]:
            inside = False
            continue
        if not inside:
            runs.append([])
            inside = True
        runs[-1].append("        %s grid=%s wg=%s lds=%s" % (
            short(r["Kernel_Name"]), r["Grid_Size_X"], r["Workgroup_Size_X"], r["LDS_Block_Size"]))
    lines = open(calls_path).read().splitlines()
    ncalls = sum(1 for l in lines if l.startswith("  "))
    if ncalls != len(runs):
        sys.exit("%d calls printed, %d runs of kernels traced" % (ncalls, len(runs)))
    # shape -> {a call's text -> [(batch, options)]}: the calls of one shape that printed and ran
    # the same are listed once
    shapes, run = {}, iter(runs)
    for l in lines:
        if l.startswith("k="):
            k, m, bb, batch = l.split(" ", 3)
            batch, opts = batch.split(" opts=")
            calls = shapes.setdefault(" ".join((k, m, bb)), {})
        else:
            tag, printed = l.split(None, 1)
            text = "\n".join(["      " + printed] + next(run))
            calls.setdefault(text, []).append((tag + " " + batch, opts))
    number = {}   # option set -> its number, in the driver's order
    for l in lines:
        if l.startswith("k="):
            number.setdefault(l.split(" opts=")[1], len(number))
    print("option sets:")
    for opts, n in number.items():
        print("  %d %s" % (n, opts))
    for shape, calls in shapes.items():
        print(shape)
        for text, cases in calls.items():
            by_batch = {}
            for batch, opts in cases:
                by_batch.setdefault(batch, []).append(number[opts])
            for batch, ns in by_batch.items():
                print("  %s opts %s" % (batch, ranges(ns)))
            print(text)


if __name__ == "__main__":
    main(*sys.argv[1:3])
