"""The host's kernel choice against the record of tests/golden/kernel_choice.json (tools/record_kernel_choice.py, taken from the commit
named in the file, before the choice became one table): every combination of tests/kernel_choice_cases.py gets the same return code, the
same rpt_last_error text and the same rpt_last_*variant / rpt_last_*exact_rcp numbers.  No combination is skipped."""
import json
import os
import time

import pytest

import kernel_choice_cases as cases

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kernel_choice.json")


def test_every_combination_chooses_as_recorded():
    """24 384 combinations on one context (frames of 128 or 576 pixels, 72 of three megapixels); measured on an MI355X: 0.2 s for the
    products, 0.9 s for the file.  Nothing is dropped from the product."""
    from relativitypathtracer_amd.renderer import Renderer
    with open(GOLDEN) as f:
        golden = json.load(f)
    products = cases.products()
    assert set(golden["products"]) == set(products)
    for name, p in products.items():          # the record is of these very axes, in this order
        assert golden["products"][name]["axes"] == json.loads(json.dumps(cases.axes_record(p))), name
    r = Renderer(0)
    try:
        t0 = time.perf_counter()
        got = cases.run_all(r)
        seconds = time.perf_counter() - t0
    finally:
        r.close()
    print(f"kernel choice: {sum(len(v) for v in got.values())} combinations in {seconds:.1f} s")
    outcomes = [tuple(o) for o in golden["outcomes"]]
    for name, p in products.items():
        index = cases.unpack_index(golden["products"][name]["index"])
        assert len(index) == len(got[name]), name
        axes = p["axes"]
        for k, (i, o) in enumerate(zip(index, got[name])):
            if outcomes[i] != o:
                where, rest = [], k             # the combination, for the message
                for axis_name, values, _ in reversed(axes):
                    where.append(f"{axis_name}={values[rest % len(values)]}")
                    rest //= len(values)
                pytest.fail(f"{name} [{', '.join(reversed(where))}]: recorded {outcomes[i]}, got {o}")
