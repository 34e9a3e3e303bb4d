"""The rollout policy's draws as a host specification (csrc/vss_policy.hip normal2).

Plain numpy, no GPU and no built library.  The kernel keys Philox4x32-10 per (row, action pair):

    key     = seed lo, seed hi
    counter = row, call counter lo, call counter hi ^ 0x504f4c00 ("POL"), action pair a = 0, 2, 4

and turns words 0 and 1 into one Box-Muller pair; words 2 and 3 are unused:

    u1  = ((w0 >> 8) + 1) 2^-24        in (0, 1]: the logarithm never sees 0
    u2  = (w1 >> 8) 2^-24              in [0, 1)
    rad = sqrt(-2 ln u1)
    ang = float32(6.2831853) * float32(u2)      one fp32 multiply, reproducible on any IEEE machine
    z[a] = rad cos(ang), z[a + 1] = rad sin(ang)

The ten rounds are vss_amd.perceive._philox, which the oracle and the GPU already pin; the keying and the
Box-Muller step are restated here in fp64 (only `ang` is rounded to fp32, so that the reference and the device
evaluate sin / cos at the same argument)."""
import numpy as np

from vss_amd.perceive import _philox

U32 = np.uint32
POL = 0x504F4C00
MASK64 = (1 << 64) - 1
TWO_PI_F32 = np.float32(6.2831853)


def policy_words(seed, counter, rows, blk):
    """The four Philox words (uint32 arrays, one entry per row) of action pair `blk` for the given rows."""
    seed, counter = int(seed) & MASK64, int(counter) & MASK64
    rows = (np.asarray(rows, dtype=np.int64) & 0xFFFFFFFF).astype(U32)
    return _philox(U32(seed & 0xFFFFFFFF), U32(seed >> 32), rows, U32(counter & 0xFFFFFFFF),
                   U32((counter >> 32) ^ POL), U32(int(blk) & 0xFFFFFFFF))


def reference_pairs(seed, counter, rows, n_act):
    """(z, rad): z (len(rows), n_act) float64 unit normals; rad (len(rows), n_act) the radius of each dim's pair."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    z = np.empty((rows.size, n_act), np.float64)
    rad = np.empty((rows.size, n_act), np.float64)
    for a in range(0, n_act, 2):
        w0, w1, _, _ = policy_words(seed, counter, rows, a)
        u1 = ((w0 >> U32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
        u2 = (w1 >> U32(8)).astype(np.float32) * np.float32(2.0 ** -24)  # exact: a 24-bit integer times 2^-24
        r = np.sqrt(-2.0 * np.log(u1))
        ang = (TWO_PI_F32 * u2).astype(np.float32).astype(np.float64)
        z[:, a], z[:, a + 1] = r * np.cos(ang), r * np.sin(ang)
        rad[:, a] = rad[:, a + 1] = r
    return z, rad


def reference_normals(seed, counter, rows, n_act):
    """(len(rows), n_act) float64: the unit normals the kernels draw for (seed, counter) at the given rows."""
    return reference_pairs(seed, counter, rows, n_act)[0]
