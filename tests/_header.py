"""include/coattn.h as text, the `coattn_*(...)` functions it declares, and the parameter list of one of them."""
import os
import re

RETURNS = r"(?:int|size_t|const char\*)"


def header():
    from vqa_amd import _lib
    return open(os.path.join(os.path.dirname(_lib.CSRC.rstrip("/")), "..", "include", "coattn.h")).read()


def declared(hdr):
    """{"coattn_forward": "int", "coattn_last_error": "const char*", ...}: every declared function and its return type."""
    return {name: ret for ret, name in re.findall(r"^(%s) (coattn_\w+)\(" % RETURNS, hdr, re.M)}


def args(hdr, name):
    """["const void* V", "int64_t v_sB", ...]: the declared parameters of `name`, whitespace normalised ([] for `(void)`)."""
    decl = re.search(r"^%s %s\(([^;]*)\);" % (RETURNS, name), hdr, re.M).group(1)
    return [] if decl.strip() == "void" else [" ".join(a.split()) for a in decl.split(",")]
