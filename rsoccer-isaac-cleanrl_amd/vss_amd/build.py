"""Build libvss_amd.so, libvss_actuate.so and libvss_estimate.so for gfx950 (hipcc cross-compiles; no GPU needed)."""
from __future__ import annotations

import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "csrc")


def build(arch: str = "gfx950", verbose: bool = False) -> str:
    out = os.path.join(HERE, "libvss_amd.so")
    cmd = ["make", "-C", CSRC, f"ARCH={arch}"]
    if not verbose:
        cmd.insert(1, "-s")
    subprocess.run(cmd, check=True)
    # the second and the third one: csrc/actuate and csrc/estimate, by the same make
    for lib in (out, os.path.join(HERE, "libvss_actuate.so"), os.path.join(HERE, "libvss_estimate.so")):
        if not os.path.exists(lib):
            raise RuntimeError(f"build did not produce {lib}")
    return out
