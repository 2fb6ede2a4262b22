"""Every kernel family's generated HIP source against
``tests/kernel_manifest.json`` (sha256 per kernel, written by
``tools/kernel_manifest.py``).  A change to the host plumbing moves
nothing here; one that means to move a kernel regenerates the file, and
its diff names the kernels touched.
"""

import importlib.util
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def _tool():
    spec = importlib.util.spec_from_file_location(
        "kernel_manifest",
        os.path.join(os.path.dirname(HERE), "tools", "kernel_manifest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_no_kernel_has_moved():
    with open(os.path.join(HERE, "kernel_manifest.json")) as fh:
        want = json.load(fh)
    got = _tool().build_manifest()
    assert len(want) > 150
    moved = sorted(k for k in want.keys() & got.keys() if want[k] != got[k])
    assert not moved, f"sources changed: {moved}"
    assert sorted(got.keys() - want.keys()) == [], "kernels not in the file"
    assert sorted(want.keys() - got.keys()) == [], "kernels no longer built"
