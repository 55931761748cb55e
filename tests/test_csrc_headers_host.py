"""The HIP sources share declarations through headers, not through hand-made copies ("Headers"): one
definition per shared struct, one buffer-descriptor constructor, no prototype of another file's function in a .hip."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "music2dance_amd", "csrc")


def _sources():
    paths = glob.glob(os.path.join(ROOT, "include", "*.h")) + glob.glob(os.path.join(CSRC, "*.h")) + \
        glob.glob(os.path.join(CSRC, "*.hip"))
    return {p: open(p).read() for p in sorted(paths)}


def test_shared_structs_are_defined_once():
    src = _sources()
    for struct in ("M2dAdamItem", "M2dWinView"):
        defs = [os.path.basename(p) for p, text in src.items() if re.search(r"\bstruct\s+%s\s*\{" % struct, text)]
        assert len(defs) == 1, (struct, defs)


def test_buffer_descriptors_come_from_the_shared_constructor():
    users = [os.path.basename(p) for p, text in _sources().items()
             if p.startswith(CSRC) and "__builtin_amdgcn_make_buffer_rsrc" in text]
    assert users == ["m2d_device.h"], users


def test_no_hip_file_declares_a_function_it_does_not_define():
    # a column-0 declaration of an m2d_* function that ends in ';' instead of a body
    proto = re.compile(r"^(?![ \t#/}])[^;{}()=]*\bm2d_\w+\s*\([^;{}]*\)\s*;", re.M)
    found = [(os.path.basename(p), m.group(0).split("(")[0]) for p, text in _sources().items() if p.endswith(".hip")
             for m in proto.finditer(text)]
    assert not found, found
