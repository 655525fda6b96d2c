"""include/coattn.h as text, and the parameter list of one of its `int coattn_*(...)` declarations."""
import os
import re


def header():
    from vqa_amd import _lib
    return open(os.path.join(os.path.dirname(_lib.CSRC.rstrip("/")), "..", "include", "coattn.h")).read()


def args(hdr, name):
    """["const void* V", "int64_t v_sB", ...]: the declared parameters of `name`, whitespace normalised."""
    decl = re.search(r"^int %s\(([^;]*)\);" % name, hdr, re.M).group(1)
    return [" ".join(a.split()) for a in decl.split(",")]
