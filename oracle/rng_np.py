"""The counter generator of rt_rng.h on numpy uint32 arrays: the one vectorised restatement the tests' references and the stage benches share.
Plain numpy, no ctypes: it needs no oracle.build().  tests/test_oracle_rng.py pins pcg4d to the oracle's scalar oracle.pcg4d."""
import numpy as np

U = np.uint32


def pcg4d(x, y, z, w):
    """Jarzynski & Olano's pcg4d.  uint32 scalars or arrays, broadcast against each other -> the four output words, each a uint32 array of the
    broadcast shape (numpy wraps mod 2^32)."""
    with np.errstate(over="ignore"):
        x, y, z, w = (np.asarray(v).astype(U) * U(1664525) + U(1013904223) for v in np.broadcast_arrays(x, y, z, w))
        x = x + y * w; y = y + z * x; z = z + x * y; w = w + y * z
        x, y, z, w = (v ^ (v >> U(16)) for v in (x, y, z, w))
        x = x + y * w; y = y + z * x; z = z + x * y; w = w + y * z
    return x, y, z, w


def path_base(k0, k1, x, s):
    return pcg4d(x, s, k0, k1)


def block_of(base, ray, j):
    """Block j of the event after ray `ray` of the paths with `base` (rt_rng.h: pcg4d(base + (0, 0, ray, j)))."""
    with np.errstate(over="ignore"):
        return pcg4d(base[0], base[1], base[2] + np.asarray(ray, U), base[3] + np.asarray(j, U))


def ctr_block(k0, k1, x, s, ray, j):
    return block_of(path_base(k0, k1, x, s), ray, j)
