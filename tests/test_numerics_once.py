"""The device numerics that the step and the three channels share exist once, in csrc/vss_numerics.h.

The kernels, vss_amd/perceive.py's numpy statement and the C oracle agree bit for bit only while every kernel runs
the same Philox, uniforms, sin / cos / log polynomials and Box-Muller.  A second definition in another kernel source
could drift from the first without any CPU test noticing; this test refuses one."""
import glob
import os
import re

from vss_amd import _native as N

SHARED = ("philox", "u01", "u01_open0", "sincos_poly", "sincos_small", "sincos_turn", "logf_poly", "box_muller", "overlap")


def test_each_shared_function_is_defined_once_in_the_numerics_header():
    sources = sorted(p for ext in ("hip", "h") for p in glob.glob(os.path.join(N.CSRC, "**", "*." + ext), recursive=True))
    assert len([p for p in sources if p.endswith(".hip")]) == 11 and os.path.join(N.CSRC, "vss_numerics.h") in sources
    for name in SHARED:
        # a definition's opening: a return type, the name, an argument list that begins with a type
        opening = re.compile(r"\b(?:void|float|bool)\s+" + name + r"\s*\(\s*(?:const\s+)?(?:uint32_t|float|void)\b")
        found = []
        for path in sources:
            with open(path) as f:
                found += [os.path.relpath(path, N.CSRC)] * len(opening.findall(f.read()))
        assert found == ["vss_numerics.h"], (name, found)


def test_the_numerics_header_is_in_every_stamp():
    """One library, one stamp: the header and the four units that include it are on the one STAMPED line."""
    for name in ("vss_numerics.h", "vss_step.hip", "vss_perceive.hip", "vss_actuate.hip", "vss_estimate.hip"):
        assert os.path.join(N.CSRC, name) in N.STAMPED, name
