"""Byte-for-byte comparison of two bench.py --dump-outputs directories.

    python tools/compare_dumps.py DIR_A DIR_B [--label TEXT]

Every DIR_A/<name>.npy must exist in DIR_B with the same shape, dtype and bytes.  Prints one line per array (bytes equal or
not; where not, the count of differing elements and the largest absolute difference) and exits 1 if any array differs or
either directory lacks one of the other's arrays.  Used for A/B runs of two library builds (bench.py --library) that must
compute the same results bit for bit."""
import argparse
import os
import sys

import numpy as np


def compare(dir_a, dir_b):
    names_a = sorted(f for f in os.listdir(dir_a) if f.endswith(".npy"))
    names_b = sorted(f for f in os.listdir(dir_b) if f.endswith(".npy"))
    lines, ok = [], bool(names_a) and names_a == names_b
    for name in sorted(set(names_a) | set(names_b)):
        if name not in names_a or name not in names_b:
            lines.append(f"{name}: only in {dir_a if name in names_a else dir_b}")
            ok = False
            continue
        a, b = np.load(os.path.join(dir_a, name)), np.load(os.path.join(dir_b, name))
        if a.shape != b.shape or a.dtype != b.dtype:
            lines.append(f"{name}: shape/dtype {a.shape} {a.dtype} vs {b.shape} {b.dtype}")
            ok = False
            continue
        if a.tobytes() == b.tobytes():
            lines.append(f"{name}: {a.shape} {a.dtype} bytes equal")
        else:
            ne = a.view(np.uint8).reshape(a.size, -1) != b.view(np.uint8).reshape(b.size, -1)
            diff = np.abs(a.astype(np.float64) - b.astype(np.float64))
            lines.append(f"{name}: {a.shape} {a.dtype} DIFFERS in {int(ne.any(axis=1).sum())} of {a.size} elements, "
                         f"max |a - b| = {float(np.nanmax(diff)) if diff.size else 0.0:.3e}")
            ok = False
    return ok, lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("dir_a")
    ap.add_argument("dir_b")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    ok, lines = compare(args.dir_a, args.dir_b)
    print(f"{args.label + ': ' if args.label else ''}{args.dir_a} vs {args.dir_b}")
    for line in lines:
        print("  " + line)
    print(f"  {'IDENTICAL' if ok else 'NOT IDENTICAL'}")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
