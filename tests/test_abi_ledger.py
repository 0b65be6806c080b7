"""A ledger of the C ABI against the suite (no GPU): every entry point include/fovealseg.h declares is named in at least one file
under tests/, or stands in EXCEPTIONS with a written reason.  A new entry point that comes without a test fails here; so does
an exception that has since got its test (the list only ever shrinks)."""
import glob
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "fovealseg.h")

# entry point -> why no test names it
EXCEPTIONS = {
    "fs_stream_wait": "orders two streams and computes nothing: every side-stream weight gradient of the training steps in "
                      "tests/test_step_invariance.py and tests/test_ddp_gloo.py goes through it (ops -> hip.stream_wait), and a "
                      "missing wait shows there as a gradient that differs between two runs",
}


def prototypes():
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)          # comments speak of entry points too
    return re.findall(r"^\s*(?:int|long)\s+(fs_\w+)\s*\(", text, flags=re.M)


def test_every_entry_point_is_named_in_a_test():
    names = prototypes()
    assert len(names) >= 141 and len(set(names)) == len(names), len(names)          # the header as it stood when the ledger was added
    assert "fs_linear_bwd_weight_bias" in names and "fs_colsum_scratch_floats" in names and "fs_set_deterministic" in names
    sources = {}
    for path in sorted(glob.glob(os.path.join(HERE, "*.py"))):
        if os.path.abspath(path) != os.path.abspath(__file__):
            with open(path) as f:
                sources[os.path.basename(path)] = f.read()
    named = {n for n in names if any(re.search(r"\b" + n + r"\b", s) for s in sources.values())}
    missing = [n for n in names if n not in named and n not in EXCEPTIONS]
    assert not missing, f"entry points of include/fovealseg.h that no file under tests/ names: {missing}"
    stale = [n for n in EXCEPTIONS if n not in names or n in named]
    assert not stale, f"EXCEPTIONS entries that are no entry point any more, or that a test names by now: {stale}"
    assert all(len(reason) > 40 for reason in EXCEPTIONS.values())
