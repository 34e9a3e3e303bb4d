"""The device numerics that the step, the channels, the set plays and the referee share exist once, in
csrc/vss_numerics.h, and what the set plays and the referee share exists once, in csrc/vss_placement.h.

The kernels, vss_amd/perceive.py's numpy statement and the C oracle agree bit for bit only while every kernel runs
the same Philox, uniforms, sin / cos / log polynomials and Box-Muller.  A second definition in another kernel source
could drift from the first without any CPU test noticing; this test refuses one."""
import glob
import os
import re

from vss_amd import _native as N

SHARED = ("philox", "u01", "u01_open0", "sincos_poly", "sincos_small", "sincos_turn", "logf_poly", "box_muller", "overlap")
PLACEMENT = ("jitter", "place_field", "store_state", "store_row", "store_team", "store_views", "play_ok", "views_ok",
             "view_spans", "outputs_alias", "outputs_overlap")


def test_each_shared_function_is_defined_once_in_the_numerics_header():
    sources = sorted(p for ext in ("hip", "h") for p in glob.glob(os.path.join(N.CSRC, "**", "*." + ext), recursive=True))
    assert len([p for p in sources if p.endswith(".hip")]) == 14 and os.path.join(N.CSRC, "vss_numerics.h") in sources
    for name in SHARED:
        # a definition's opening: a return type, the name, an argument list that begins with a type
        opening = re.compile(r"\b(?:void|float|bool)\s+" + name + r"\s*\(\s*(?:const\s+)?(?:uint32_t|float|void)\b")
        found = []
        for path in sources:
            with open(path) as f:
                found += [os.path.relpath(path, N.CSRC)] * len(opening.findall(f.read()))
        assert found == ["vss_numerics.h"], (name, found)


def test_the_placement_is_defined_once_in_the_placement_header():
    """World and every function that vss_setplay.hip and vss_referee.hip share: in vss_placement.h and in no .hip."""
    sources = sorted(p for ext in ("hip", "h") for p in glob.glob(os.path.join(N.CSRC, "**", "*." + ext), recursive=True))
    assert os.path.join(N.CSRC, "vss_placement.h") in sources
    for name in PLACEMENT + ("World",):
        # a definition's opening: `struct World {`, or a return type, the name and an argument list that begins with a type
        opening = re.compile(r"\bstruct\s+World\s*\{" if name == "World" else
                             r"\b(?:void|float|bool)\s+" + name + r"\s*\(\s*(?:const\s+)?(?:uint32_t|int32_t|int64_t|float|void|vss_\w+)\b")
        found = []
        for path in sources:
            with open(path) as f:
                found += [os.path.relpath(path, N.CSRC)] * len(opening.findall(f.read()))
        # the three row channels each have a store_row of their own: another function, of a channel's row
        own = ["vss_estimate.hip", "vss_perceive.hip", "vss_track.hip"] if name == "store_row" else []
        assert sorted(found) == sorted(own + ["vss_placement.h"]), (name, found)


def test_the_numerics_header_is_in_every_stamp():
    """One library, one stamp: the two headers and the units that include them are on the one STAMPED line."""
    for name in ("vss_numerics.h", "vss_step.hip", "vss_perceive.hip", "vss_actuate.hip", "vss_estimate.hip", "vss_track.hip",
                 "vss_setplay.hip", "vss_referee.hip", "vss_placement.h"):
        assert os.path.join(N.CSRC, name) in N.STAMPED, name
    for name in ("vss_track.hip", "vss_setplay.hip", "vss_referee.hip", "vss_placement.h"):
        with open(os.path.join(N.CSRC, name)) as f:
            assert '#include "vss_numerics.h"' in f.read(), name
