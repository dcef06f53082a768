#!/usr/bin/env python3
"""Record which kernel (or which refusal) the host chooses for every combination of tests/kernel_choice_cases.py, on the library as built.

    python tools/record_kernel_choice.py --commit <hash of the commit the library was built from> [--out tests/golden/kernel_choice.json]

The file is a table of the distinct outcomes and, per product, one index into it per combination in the order of the product's axes (the
first axis outermost): little-endian uint16, zlib, base64 (kernel_choice_cases.pack_index / unpack_index).
tests/test_gpu_kernel_choice.py compares the code under test with it: record it from the commit BEFORE a change to the kernel choice,
never from the change itself."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", required=True, help="the commit the library under record was built from (stored in the file)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "kernel_choice.json"))
    args = ap.parse_args()
    import kernel_choice_cases as cases
    from relativitypathtracer_amd.renderer import Renderer
    r = Renderer(0)
    t0 = time.perf_counter()
    results = cases.run_all(r)
    seconds = time.perf_counter() - t0
    r.close()
    outcomes, index_of = [], {}
    record = {"commit": args.commit, "outcomes": outcomes, "products": {}}
    for name, product in cases.products().items():
        idx = []
        for o in results[name]:
            if o not in index_of:
                index_of[o] = len(outcomes)
                outcomes.append(list(o))
            idx.append(index_of[o])
        record["products"][name] = {"axes": cases.axes_record(product), "index": cases.pack_index(idx)}
    with open(args.out, "w") as f:
        json.dump(record, f, separators=(",", ":"))
        f.write("\n")
    n = sum(len(v) for v in results.values())
    print(f"{n} combinations, {len(outcomes)} distinct outcomes, {seconds:.1f} s, {os.path.getsize(args.out)} bytes -> {args.out}")


if __name__ == "__main__":
    main()
