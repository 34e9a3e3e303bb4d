"""Build libvss_amd.so, libvss_track.so, libvss_setplay.so and libvss_referee.so for gfx950 (hipcc cross-compiles; no GPU needed)."""
from __future__ import annotations

import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "csrc")


def build(arch: str = "gfx950", verbose: bool = False) -> str:
    out = os.path.join(HERE, "libvss_amd.so")
    cmd = ["make", "-C", CSRC, f"ARCH={arch}"]  # csrc/Makefile runs csrc_track/, csrc_setplay/ and csrc_referee/Makefile as well
    if not verbose:
        cmd.insert(1, "-s")
    subprocess.run(cmd, check=True)
    for lib in (out, os.path.join(HERE, "libvss_track.so"), os.path.join(HERE, "libvss_setplay.so"),
                os.path.join(HERE, "libvss_referee.so")):
        if not os.path.exists(lib):
            raise RuntimeError(f"build did not produce {lib}")
    return out
